// libmocr_hip.so - engine and C ABI (include/mocr.h) of the MI355X-native Manga-OCR recogniser.
//
// Data flow of one batch of n crops (M = n * 197 encoder rows), all buffers resident in HBM:
//
//   gray u8 [n,224,224] --patchify--> Ape T[n*196,256] --GEMM+bias+pos--> X f32 [M,768]   (CLS rows apart)
//   12 x { LN(X)->Xn T ; QKV GEMM ->QKV T[M,2304] ; attention -> CTX T[M,768] ; O GEMM + resid -> X ;
//          LN(X)->Xn ; FC1 GEMM+GELU -> Hb T[M,3072] ; FC2 GEMM + resid -> X }
//   LN(X) -> ENC T[M,768] ; cross-K/V GEMM (both decoder layers at once) -> CKV T[M, 2*2*768]
//   greedy loop, <= max_len-1 steps over n rows: see decode_step().
//
// The residual stream X is fp32 in both modes; T is the storage type of GEMM operands
// (bf16 or fp32).  Decode-step projections (M = n) are split-K GEMMs writing fp32 partial slabs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/mocr.h"
#include "common.h"
#include "kernels_attn.h"
#include "kernels_decode.h"
#include "kernels_gemm.h"
#include "kernels_gemm_pers.h"
#ifdef MOCR_EXPERIMENTS
#include "kernels_gemm_lab.h"      // A/B kernels of earlier rounds: not in the product library
#endif
#include "kernels_latent.h"
#include "kernels_latent8.h"
#include "kernels_latent_t.h"
#include "kernels_latent_t8.h"
#include "kernels_smallm.h"
#include "preprocess.h"
#include "prep_pipeline.h"
#include "kernels_qqt.h"
#include "kernels_misc.h"
#include "kernels_positions.h"
#include "kernels_share.h"
#include "kernels_beam.h"

namespace {

struct HipError { hipError_t code; const char* what; int line; };
#define HIPCHECK(x)                                             \
    do {                                                        \
        hipError_t err__ = (x);                                 \
        if (err__ != hipSuccess) throw HipError{err__, #x, __LINE__}; \
    } while (0)
struct ArgError { std::string msg; int code; };

static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

static inline uint16_t host_f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static inline float host_bf2f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct EncLayerW {
    void *wqkv, *wo, *w1, *w2;
    float *bqkv, *bo, *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b;
    // bf16 engines, LayerNorm folded into the GEMM behind it (gemm_pers_kernel LNF): W o gamma, its column sums (of the
    // bf16-rounded values), b + W beta
    void *wqkv_f = nullptr, *w1_f = nullptr;
    float *sqkv = nullptr, *s1 = nullptr, *bqkv_f = nullptr, *b1_f = nullptr;
};
struct DecLayerW {
    void *wqkv, *wo, *wqc, *woc, *w1, *w2;
    void *wkT_s = nullptr, *wkT_c = nullptr;   // latent attention: (Wk^T)/8 of the self / cross attention, [768 in][768 out]
    float *bqkv, *bo, *bqc, *boc, *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b, *ln3g, *ln3b;
};
struct Weights {
    void* wpe = nullptr; float *bpe = nullptr, *cls = nullptr, *pos_enc = nullptr;
    std::vector<EncLayerW> enc;
    float *lnfg = nullptr, *lnfb = nullptr;
    void* wckv = nullptr; float* bckv = nullptr;
    float *word = nullptr, *posd = nullptr, *type0 = nullptr, *embg = nullptr, *embb = nullptr;
    std::vector<DecLayerW> dec;
    void* wt = nullptr; float *bt = nullptr, *lntg = nullptr, *lntb = nullptr;
    void* wv = nullptr; float* bv = nullptr;
    float* lut = nullptr;
    float* zero_bias = nullptr;
    // fp8 attention (MOCR_FLAG_FP8_ATTENTION): static e4m3 scales of the key/value sources (x = x8 * sx)
    float sx_enc = 1.f;                 // encoder output = LayerNorm_f
    std::vector<float> sx_self;         // per decoder layer: its input rows (embedding LayerNorm / previous layer's LayerNorm 3)
};

struct ProfRec { int kid; hipEvent_t e0, e1; double flops, bytes; };

}  // namespace

// Everything one in-flight batch needs: a HIP stream and its own workspace.  The engine keeps
// `lanes` of them (the counterpart of the reference's pool of QueueProcessorWorker threads,
// src/ui/main_window.py:4286-4327): independent batches overlap on the GPU, which is what fills
// the chip during the latency-bound decode steps.  Host code runs single-threaded under the
// engine mutex and "binds" one lane at a time: mocr_engine derives from LaneCtx, and bind()
// copies the lane's pointers into that base, so the launch code simply says e->X, e->stream.
struct LaneCtx {
    int lane_id = 0;
    hipStream_t stream = nullptr;
    uint8_t *d_in = nullptr, *d_rgb = nullptr;
    float* X = nullptr;
    void *Xn = nullptr, *QKV = nullptr, *CTX = nullptr, *Hb = nullptr, *ENC = nullptr, *CKV = nullptr;
    float* ln_part = nullptr;                  // [Mp][4][2] row statistics partials of X (LayerNorm folded into the encoder GEMMs)
    void *kcache = nullptr, *vcache = nullptr;     // [dec_layers][Bp][H][max_len][64]
    float* slabs = nullptr; long long slab_cap = 0; // floats
    float* cand_val = nullptr; int* cand_idx = nullptr;   // [Bp][vocab/64] per-tile argmax candidates of the LM head
    float* cand_sum = nullptr;                      // [Bp][vocab/64] scored batches: per-tile sum of exp(logit - the tile's max)
    float* scores = nullptr;                        // [Bp][max_len] scored batches: log-probability of every emitted token, by row like ids
    // token alternatives: allocated by the first batch that asks (ensure_alt_buffers), so other engines keep their footprint
    float* top_val = nullptr; int* top_idx = nullptr;   // [Bp][vocab/64][4] per-tile four best logits / columns of the LM head
    int* alt_ids = nullptr; float* alt_logp = nullptr;  // [Bp][max_len][4] the four best tokens of every step / their log-probabilities, by row like ids
    // token constraints: allocated by the first constrained batch (ensure_set_buffer)
    int* set_of_row = nullptr;                      // [Bp] constrained batches: the token set of every row, by row like ids
    // no-repeat n-grams: allocated by the first batch with a row of n > 0 (ensure_ngram_buffers)
    unsigned* row_mask = nullptr;                   // [Bp][V / 32] the effective set of every row's next step (base set minus the bans), by row
    int* row_ident = nullptr;                       // [Bp] 0, 1, 2, ...: the "set of every row" that makes the masked kernels read row_mask[row]
    int* ngram_of_row = nullptr;                    // [Bp] no_repeat_ngram_size of every row (0: off), by row
    // token automata: allocated by the first batch with a row that brings one (ensure_automaton_buffers)
    int* aut_base_of_row = nullptr;                 // [Bp] the global number of every row's start state (-1: no automaton), by row
    int* aut_state = nullptr;                       // [Bp] the global state every row is in (AUT_STATE_NONE / AUT_STATE_DEAD), by row
    int* aut_state_out = nullptr;                   // [Bp] ... in the automaton's own numbering: what the jobs' out_state receives
    // repetition penalty: allocated by the first batch with a row of p != 1 (ensure_penalty_buffers)
    unsigned* seen_mask = nullptr;                  // [Bp][V / 32] the tokens every row holds (start, forced, chosen), by row
    float* penalty_of_row = nullptr;                // [Bp] repetition_penalty of every row (1: off), by row
    // token positions: allocated by the first batch that asks (ensure_pos_buffers)
    void* pos_hist = nullptr;                      // [Bp][max_len][768] T (+ one GEMM tile of rows): the last layer's LayerNorm-1 output of every
                                                    // (row, input position), by row like ids - what the cross-attention query projection read.
                                                    // A batch packs it as [rows][its generate(max_length)][768]
    float* pos_out = nullptr;                       // [Bp][max_len][MOCR_POSITION_FIELDS] by row like ids
    void *pos_q = nullptr, *pos_k = nullptr;        // deferred pass: queries / keys of POS_CHUNK rows at a time
    // forced prefixes: allocated by the first batch that asks (ensure_prefix_buffers)
    int* prefix = nullptr;                          // [Bp][max_len] the caller-given tokens of every row (without the start token), by row like ids
    int* prefix_len = nullptr;                      // [Bp] by row (0: none)
    float* tgt_val = nullptr;                       // [Bp] by slot: the LM head's value of the step's forced column
    // shared encodings: allocated by the first batch with a job that shares (ensure_share_buffer)
    int* src_of_row = nullptr;                      // [Bp] the encoder row (crop of the batch) every decode row reads, by row like ids
    size_t ctx_cap = 0;                             // bytes CTX was allocated with: a sharing batch stages its encodings there (expand_encodings)
    // beam search: allocated by the first beam batch (ensure_beam_buffers); all by row like ids (kernels_beam.h: BeamState)
    float *beam_score = nullptr, *hyp_score = nullptr;    // [Bp]
    int *beam_parent = nullptr, *hyp_len = nullptr, *heuristic_open = nullptr;      // [Bp] ([Bp / 2] used of the last)
    int* hyp_ids = nullptr;                         // [Bp][max_len]
    // ... and its token form: allocated by the first beam batch that asks for token scores or brings a token set
    // (ensure_beam_token_buffers); the rows' sets are set_of_row
    float *beam_logp = nullptr, *hyp_logp = nullptr;    // [Bp][max_len]
    // ... and its trail form: allocated by the first beam batch that asks for token positions (ensure_beam_position_buffers)
    uint8_t *beam_trail = nullptr, *hyp_trail = nullptr;    // [Bp][max_len]
    // ... and its automaton form: allocated by the first beam batch that brings a token automaton (ensure_beam_automaton_buffers);
    // the running beams' states are aut_state, the crops' start states aut_base_of_row
    int* hyp_state = nullptr;                       // [Bp] the global state of every finished hypothesis (AUT_STATE_NONE: none), by row
    float *x_f32 = nullptr, *a_f32 = nullptr, *c_f32 = nullptr;
    float* ln_stats = nullptr;                      // small-batch path: (mean, rstd) per row of the three pre-LayerNorm sums, [3][Bp][2]
    void *x_t = nullptr, *a_t = nullptr, *c_t = nullptr, *ctx_t = nullptr, *h_t = nullptr, *z_t = nullptr;
    int *ids = nullptr, *step = nullptr, *finished = nullptr, *len = nullptr, *n_unf = nullptr;
    int* forced = nullptr; float* logits_dbg = nullptr; size_t forced_cap = 0, logits_cap = 0;
    int* h_pinned = nullptr;                        // [4] pinned: early-exit flags
    // latent attention (bf16): q [Bp,768], Qt / Et [Bp,16,768], per-layer input rows [layers][Bp][max_len][768]
    void *q_t = nullptr, *qt = nullptr, *et = nullptr, *xcache = nullptr;
    int* rowmap = nullptr;                          // [Bp] decode slot -> row of the batch (identity until the batch is compacted)
    int* rowmap_tmp = nullptr;                      // [2][Bp] compaction scratch: the new map, and every new slot's old slot
    // fp8 attention: e4m3 copies of the encoder output [Mp][768] and of the per-layer input rows [layers][Bp][max_len][768]
    uint8_t *enc8 = nullptr, *x8cache = nullptr;
};

// One recognise request of <= max_batch crops.
struct Job {
    hipEvent_t wait_ev = nullptr;   // device planes that a preparation stream is still writing: the lane's stream waits for this first
    const uint8_t* src = nullptr;   // host images (src_host) or device luminance planes
    bool src_host = false;
    int channels = 1;
    int64_t row_stride = 0, image_stride = 0;
    int n = 0, max_len = 0;         // decode rows
    // shared encodings (the *_shared entry points): the job brings n_src planes, row r reads plane src_of_row[r] of them
    // (empty: every row its own plane, n_src == n); `planes`: where they lie behind `src`, in planes (empty: 0, 1, 2, ...)
    int n_src = 0;
    std::vector<int32_t> src_of_row, planes;
    int32_t* out_ids = nullptr;     // host (out_host) or device
    int32_t* out_len = nullptr;
    float* out_logp = nullptr;      // nullable: [n][max_len] token log-probabilities (the *_scored entry points); host or device like out_ids
    int32_t* out_alt_ids = nullptr; // nullable, both or neither (the *_alts entry points): [n][max_len][MOCR_ALTERNATIVES] the four best tokens of
    float* out_alt_logp = nullptr;  // every position and their log-probabilities; host or device like out_ids
    bool out_host = false;
    std::vector<int32_t> sets;      // token constraints (the *_constrained entry points): one set handle per crop; empty = all MOCR_TOKEN_SET_ALL
    std::vector<int32_t> ngram;     // no-repeat n-grams (the *_norepeat entry points): one size per crop; empty = all 0
    std::vector<int32_t> automata;  // token automata (the *_automaton entry points): one handle per row; empty = all MOCR_AUTOMATON_NONE
    int32_t* out_state = nullptr;   // nullable: [n] the rows' final automaton states; host or device like out_ids
    std::vector<float> penalty;     // repetition penalty (the *_penalty entry points): one p per row; empty = all 1
    float* out_pos = nullptr;      // nullable (the *_positions entry points): [n][max_len][MOCR_POSITION_FIELDS]; host or device like out_ids
    std::vector<int32_t> prefix_len;    // forced prefixes (the *_prefix entry points): one length per crop; empty = all 0
    std::vector<int32_t> prefix;        // ... and the tokens, [n][prefix_ld] (a copy: the caller's arrays need not outlive the call)
    int prefix_ld = 0;
    // beam search (the *_beam entry points; beam.num_beams = 0: a greedy job): n = crops x K rows that share the crops'
    // encodings, out_ids / out_len receive the finished hypotheses [crops][K] and out_score their scores
    mocr_beam_config beam{};
    float* out_score = nullptr;
};

static bool same_beam(const mocr_beam_config& a, const mocr_beam_config& b) {
    return a.num_beams == b.num_beams && a.length_penalty == b.length_penalty && a.early_stopping == b.early_stopping &&
           a.no_repeat_ngram_size == b.no_repeat_ngram_size;
}

// The kind of decode steps a batch runs: the richest of what its jobs asked for.  Every choice that follows from it - the
// LM-head epilogue, the token kernel, the profile names, the decode-graph key - is made from this one value.
struct DecMode {
    int level = 0;                  // 0 ids only, 1 token log-probabilities (the scored LM head / token kernel), 2 also the token
                                    // alternatives (EPI_TOPK / the TOPK token kernel)
    bool mask = false;              // a row decodes under a token set other than MOCR_TOKEN_SET_ALL (or `ngram`): the steps run the
                                    // masked (EPI_*_M / MASK) form of the level's LM head and token kernel
    bool ngram = false;             // a row has no_repeat_ngram_size > 0: the masks are the per-row ones (row_mask through row_ident)
                                    // and the token kernel is the NGRAM one, which rebuilds them
    bool automaton = false;         // a row brings a token automaton (implies `ngram`: the same per-row masks): the token kernel is the
                                    // AUTOMATON one, which also walks the rows' states, and the batch starts with automaton_init_kernel
    bool soft = false;              // ... and one of those automata is SOFT (edge weights / open states; implies `automaton`): the LM head is the
                                    // SOFT form of the masked epilogue, the token kernel the SOFT one, the batch starts with
                                    // automaton_init_kernel<true>
    bool penalty = false;           // a row has a repetition penalty p != 1 (implies `soft`, so that the build has one more family and not two:
                                    // rows without an automaton read state NONE and add nothing): the LM head and the token kernel are the
                                    // PEN forms, the batch also starts with penalty_init_kernel
    bool positions = false;        // a job asked for token positions: the steps record pos_hist, finish_batch runs the deferred pass
                                    // (a beam batch too: its selection then also keeps the beam-index trails the pass gathers by)
    bool prefix = false;            // a row has a forced prefix: the steps run scored and masked (level >= 1, mask; unconstrained rows read
                                    // set 0), the LM head also leaves the forced column's value and the token kernel stores the forced token
    bool beam = false;              // a beam-search batch (all of its jobs, with one configuration): the steps end in the selection and
                                    // the cache reorder instead of the token kernel, the LM head always in its slab form
    mocr_beam_config beam_cfg{};
    bool beam_tokens = false;       // ... in which a job asks for token scores or brings a token set other than MOCR_TOKEN_SET_ALL: the
                                    // selection runs in its token form (level and mask stay 0: the LM head and the caches do not change)
    bool beam_automaton = false;    // ... in which a job brings a token automaton other than MOCR_AUTOMATON_NONE (implies beam_tokens): the
                                    // selection runs in its automaton form and the batch starts with beam_automaton_init_kernel; with
                                    // `soft` (one of those automata is soft) in its SOFT form, on the arena's weights and default edges
    // a graph captured in one mode is never replayed in another: the mode's share of the decode-graph key (6 bits; a beam
    // batch: bit 6, its token form: bit 7, an automaton batch: bit 8, a beam batch's automaton form: bit 9, a soft automaton
    // batch: bit 10, a penalty batch: bit 11, and a beam batch's configuration - kernel arguments of the captured launches - in
    // the bits above, beam_key)
    int key_bits() const {
        return level + (mask ? 4 : 0) + (ngram ? 8 : 0) + (positions ? 16 : 0) + (prefix ? 32 : 0) + (beam ? 64 : 0) + (beam_tokens ? 128 : 0) +
               (automaton ? 256 : 0) + (beam_automaton ? 512 : 0) + (soft ? 1024 : 0) + (penalty ? 2048 : 0);
    }
    static constexpr int KEY_SPAN = 4096;
    int epilogue() const { return mask ? (level == 2 ? EPI_TOPK_M : level == 1 ? EPI_ARGMAX_LSE_M : EPI_ARGMAX_M)
                                       : (level == 2 ? EPI_TOPK : level == 1 ? EPI_ARGMAX_LSE : EPI_ARGMAX); }
    // profile name of the fused LM head (the token kernel's is its form's: TokenFamily)
    const char* head_name() const {
        return penalty ? "gemm_dec_vocab_rp" : soft ? "gemm_dec_vocab_sw" : mask ? "gemm_dec_vocab_m" : level == 2 ? "gemm_dec_vocab_topk" : level == 1 ? "gemm_dec_vocab_lse" : "gemm_dec_vocab";
    }
};

static DecMode mode_of(const std::vector<Job>& jobs) {
    DecMode m;
    // beam search: pump_once never mixes - a batch is all beam jobs of one configuration, or has none.  Its jobs' token
    // scores and sets are the selection's business alone (the token form), not the LM head's.
    if (!jobs.empty() && jobs.front().beam.num_beams > 0) {
        m.beam = true; m.beam_cfg = jobs.front().beam;
        for (const Job& j : jobs) {
            m.beam_tokens = m.beam_tokens || j.out_logp || !j.sets.empty();
            m.positions = m.positions || j.out_pos;
            m.beam_automaton = m.beam_automaton || !j.automata.empty();     // (slice_rows: MOCR_AUTOMATON_NONE alone comes as empty)
        }
        m.beam_tokens = m.beam_tokens || m.beam_automaton;
        return m;
    }
    for (const Job& j : jobs) {
        m.level = std::max(m.level, j.out_alt_ids ? 2 : j.out_logp ? 1 : 0);
        for (int32_t h : j.sets) m.mask = m.mask || h != MOCR_TOKEN_SET_ALL;
        for (int32_t g : j.ngram) m.ngram = m.ngram || g > 0;
        m.automaton = m.automaton || !j.automata.empty();      // (slice_rows: an array of MOCR_AUTOMATON_NONE alone comes as empty)
        m.positions = m.positions || j.out_pos;
        m.prefix = m.prefix || !j.prefix_len.empty();
        m.penalty = m.penalty || !j.penalty.empty();            // (slice_job: rows of p = 1 alone come as empty)
    }
    if (m.penalty) m.soft = m.automaton = true;     // the PEN forms are SOFT forms: rows without an automaton are in state NONE
    m.ngram = m.ngram || m.automaton;           // an automaton's sets reach the step through the same per-row masks
    if (m.prefix) m.level = std::max(m.level, 1);      // a forced token is one more per-row fact of the masked, scored step
    m.mask = m.mask || m.ngram || m.prefix;     // the bans are applied through the rows' masks, which start as the rows' sets
    return m;
}

struct Lane {
    LaneCtx ctx;
    bool active = false;
    std::vector<Job> jobs;          // requests merged into this lane's current batch, in row order
    int n = 0, max_len = 0;         // rows of the merged batch, its generate(max_length)
    int n_enc = 0;                  // crops the encoder runs on: the jobs' planes (n unless a job shares encodings)
    std::vector<int> h_src;         // the upload of src_of_row stages from here
    int np = 0;                     // slots the decode steps run on: n rounded up (graph_rows), the extra ones are born finished; shrinks when the batch is compacted
    int np0 = 0;                    // np at the start of the batch = its kernel regime
    DecMode mode;                   // mode_of(jobs)
    std::vector<int> h_sets, h_ngram;   // the uploads of set_of_row / ngram_of_row stage from here
    std::vector<int> h_plen, h_prefix;  // ... and those of prefix_len / prefix
    std::vector<int> h_aut;             // ... and that of aut_base_of_row
    std::vector<float> h_penalty;       // ... and that of penalty_of_row
    int t = 0, steps = 0, chunk = 0;
    bool finishing = false;         // a flag of this batch has reported a finished row: rows are leaving, chunks get shorter
    bool flag_pending[2] = {false, false};
    hipEvent_t flag_ev[2] = {nullptr, nullptr};
};

struct mocr_engine : LaneCtx {
    mocr_config cfg{};
    std::string err;
    std::mutex mu;
    std::mutex err_mu;              // guards err: mocr_last_error may be called while another thread fails
    std::atomic<bool> poisoned{false};   // a HIP call failed: HIP errors are sticky, so every later call is refused (read without the mutex)
    bool committed = false;
    int gen_max_len = 0;            // generate(max_length) of the device-buffer submissions (mocr_set_generate_max_length)
    bool fp8attn = false;           // latent attention on e4m3 key/value rows + fp8 MFMA (MOCR_FLAG_FP8_ATTENTION, opt-in)
    bool latent = false;            // bf16 engines: latent (absorbed) decode attention ...
    int classic_rows = 0;           // ... for batches of more than this many rows; smaller ones use the classic kernels
    // LayerNorm folding (bf16, persistent encoder GEMMs) is gated by a measurement on THIS checkpoint (calibrate_ln_fold):
    // the fold feeds bf16(x) - the raw residual stream - into the matrix cores where the launches feed bf16(LN(x)); per row
    // the input-rounding noise of the two forms is in the ratio sqrt(sum (x g rstd)^2 / sum (LN(x))^2), ~1 on a
    // near-normalised stream and |mean| / spread on a stream with a DC offset.
    struct FoldCalib { std::vector<std::vector<float>> g, b; size_t idx = 0; double worst = 0.0; std::vector<float> hx; };
    FoldCalib* calib = nullptr;     // non-null only inside calibrate_ln_fold
    bool fold_ok = true;            // the measured ratio allows the fold (<= FOLD_RATIO_MAX on every LayerNorm input)
    float fold_ratio = 0.f;         // the worst ratio measured (0: not measured)
    long long n_slot_steps = 0;     // decode slots x steps enqueued so far (mocr_decode_slot_steps): what the steps cost, in rows
    long long n_compactions = 0;    // batches whose rows were compacted, counted per compaction (mocr_compaction_count)
    long long n_encoded = 0;        // crops the recognise calls' batches have put through the encoder (mocr_encoded_crops)
    int lat_tk = 18;                // bf16 latent attention kernel: 18 = latent_attnT_kernel, three blocks per CU (default); 32 = latent_attn_kernel on 32-key tiles; experiments: 17, 16
    int Bc = 0;                     // rows the classic K/V buffers are sized for
    // Kernel regime of the batch being decoded: the row count the batch STARTED with (0: the launch's own row count).
    // Every choice a decode step makes by row count - attention path, GEMM tile, split-K slabs, fused query kernel,
    // cache policy - is made by rrows(n), so a batch whose rows were compacted (r04: fewer slots per step as rows finish)
    // keeps the summation order it started with and a row's ids do not depend on when its neighbours finished.
    int regime = 0;
    int rrows(int n) const { return regime > 0 ? regime : n; }
    bool use_latent(int n) const { return latent && n > classic_rows; }
    // bf16: greedy batches of up to this many rows take the one-launch-per-projection path (kernels_smallm.h); a beam batch
    // never does - whoever asks about one says !DecMode::beam first
    int smallm_rows = 0;
    bool use_smallm(int n) const { return n <= smallm_rows && !use_latent(n); }
    std::vector<mocr_beam_config> beam_cfgs;    // the beam configurations seen: a decode graph bakes one in, its key names it by index
    std::map<std::string, std::vector<float>> host_w;
    std::map<std::string, std::vector<int64_t>> host_shape;
    std::vector<void*> allocs;
    Weights w;
    // geometry
    int S = 0, G = 0, D = 0, H = 0, F = 0, V = 0, Bp = 0, Mp = 0, NCKV = 0;
    int num_cus = 256;           // compute units, rounded down to a multiple of 8 (persistent grids: equal share per XCD)
    size_t esz = 2;
    std::vector<Lane> lanes;
    std::vector<Job> pending;
    // token sets (mocr_token_set_create): immutable rows of a device bit table [MOCR_MAX_TOKEN_SETS][V / 32], row 0 all ones;
    // the table is allocated by the first set, the host copies serve the lookup by content and the handle check
    unsigned* tok_table = nullptr;
    std::vector<std::vector<uint32_t>> tok_sets;
    std::map<std::vector<uint32_t>, int> tok_index;
    // token automata (mocr_automaton_create): one device arena in CSR form over global state numbers, allocated at full
    // capacity by the first create so that its addresses - kernel arguments of captured decode graphs - never move; a new
    // automaton is appended behind the last.  aut_first[h] / aut_states[h]: handle h's first global state and state count
    // (handle 0 = MOCR_AUTOMATON_NONE holds nothing)
    int *aut_edge_begin = nullptr, *aut_edge_token = nullptr, *aut_edge_next = nullptr;
    uint8_t* aut_accepting = nullptr;
    // ... and its soft part, allocated at full capacity by the first create of a SOFT automaton and
    // pre-filled with weight 0 / default -1, which is what every automaton created without the two arrays reads there
    float* aut_edge_weight = nullptr;
    int* aut_default_next = nullptr;
    std::vector<char> aut_soft{0};      // by handle: the automaton brought edge_weight or default_next
    std::vector<int> aut_first{0}, aut_states{0};
    int aut_n_states = 0, aut_n_edges = 0;
    // decode-step HIP graphs, keyed by (lane, rows, (max_len, context bucket, DecMode::key_bits), steps per graph)
    std::map<std::tuple<int, int, long long, int, int>, hipGraphExec_t> graphs;      // + the regime
    void bind(int i) { static_cast<LaneCtx&>(*this) = lanes[i].ctx; }
    void unbind(int i) { lanes[i].ctx = static_cast<LaneCtx&>(*this); }
    // device preprocessing (preprocess.h): resample tables per input size, grow-only scratch
    std::map<int, ResampleTable> rs_tables;
    struct Scratch { void* p = nullptr; size_t cap = 0; };
    Scratch rs_src, rs_tmp, rs_desc, rs_coef, rs_bounds, rs_gray;
    // PINNED host staging of the packed pixel rows (grow-only): the H2D copy is one DMA at link speed.  Two buffers: the
    // host packs chunk k + 1 into one while the copy engine reads chunk k from the other (prepare_and_decode).
    Scratch rs_pin[2];
    hipStream_t prep_stream = nullptr;      // pack -> H2D -> resize of the host entry points: never a lane's stream
    void* grow_pinned(int slot, size_t bytes) {
        Scratch& sp = rs_pin[slot & 1];
        if (bytes > sp.cap) {
            if (sp.p) HIPCHECK(hipHostFree(sp.p));
            sp.p = nullptr; sp.cap = 0;
            const size_t cap = std::max<size_t>(bytes + bytes / 2, 1 << 20);
            HIPCHECK(hipHostMalloc(&sp.p, cap, hipHostMallocDefault));
            sp.cap = cap;
        }
        return sp.p;
    }
    void* grow(Scratch& s, size_t bytes) {
        if (bytes > s.cap) {
            if (s.p) HIPCHECK(hipFree(s.p));
            s.p = nullptr; s.cap = 0;
            const size_t cap = std::max<size_t>(bytes + bytes / 2, 4096);
            HIPCHECK(hipMalloc(&s.p, cap));
            s.cap = cap;
        }
        return s.p;
    }
    // profiling
    bool prof_on = false;
    std::vector<std::string> knames;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> ev_pool;
    std::vector<mocr_kernel_stat> stats;

    template <typename X_> X_* dalloc(size_t count) {
        void* p = nullptr;
        HIPCHECK(hipMalloc(&p, std::max<size_t>(count * sizeof(X_), 256)));
        HIPCHECK(hipMemset(p, 0, std::max<size_t>(count * sizeof(X_), 256)));
        // the fill runs on the null stream, which the lanes' non-blocking streams do not wait for: a buffer
        // allocated lazily (test hooks) could otherwise be zeroed AFTER its first asynchronous upload
        HIPCHECK(hipDeviceSynchronize());
        allocs.push_back(p);
        return reinterpret_cast<X_*>(p);
    }
    int kid(const char* name) {
        for (size_t i = 0; i < knames.size(); ++i)
            if (knames[i] == name) return (int)i;
        knames.push_back(name);
        mocr_kernel_stat s{};
        snprintf(s.name, sizeof(s.name), "%s", name);
        stats.push_back(s);
        return (int)knames.size() - 1;
    }
    hipEvent_t get_event() {
        if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
        hipEvent_t e; HIPCHECK(hipEventCreate(&e)); return e;
    }
    void prof_begin(const char* name, double flops, double bytes) {
        if (!prof_on) return;
        ProfRec r{kid(name), get_event(), get_event(), flops, bytes};
        HIPCHECK(hipEventRecord(r.e0, stream));
        recs.push_back(r);
    }
    void prof_end() {
        if (!prof_on) return;
        HIPCHECK(hipEventRecord(recs.back().e1, stream));
    }
    void prof_collect() {
        if (recs.empty()) return;
        HIPCHECK(hipDeviceSynchronize());
        for (auto& r : recs) {
            float ms = 0.f;
            HIPCHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
            auto& s = stats[r.kid];
            s.launches += 1; s.total_ms += ms; s.flops += r.flops; s.bytes += r.bytes;
            ev_pool.push_back(r.e0); ev_pool.push_back(r.e1);
        }
        recs.clear();
    }
};

namespace {

struct ProfScope {
    mocr_engine* e;
    ProfScope(mocr_engine* e_, const char* name, double flops, double bytes) : e(e_) { e->prof_begin(name, flops, bytes); }
    ~ProfScope() { e->prof_end(); }
};

// Tuning knobs: the MOCR_* environment overrides exist in the experiments build only (-DMOCR_EXPERIMENTS,
// `python manga-ocr_amd/build.py --experiments`, used by tools/); the product library runs the measured defaults and
// reads no environment variable in its launch code.
#ifdef MOCR_EXPERIMENTS
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}
#define LAB_ONLY(...) __VA_ARGS__      // rows of a table that exist in the experiments build only
#else
static constexpr int env_int(const char*, int dflt) { return dflt; }
#define LAB_ONLY(...)
#endif

template <typename K> void set_max_lds(K kernel, int bytes) {
    HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}

// ---------------------------------------------------------------------------------------- kernel families
// A kernel template that is built in several forms has ONE table, `forms`: each row is a set of template arguments (a literal
// struct, `Args`) and nothing else.  Row I gives the instantiation (kernel<I>()) and the dynamic LDS it may use (lds(row)), and
// the row itself is the run-time key a launch asks for.  A launch walks its family's table (find_form) and init_kernel_attrs
// walks the same tables (raise_lds): what is launched is listed, what is listed is built, and no other line names a form.
template <typename Kernel> struct Form {
    Kernel kernel = nullptr;      // null: the family has no such form
    int lds = 0;
};

// Forms whose trailing argument differs in TYPE (GemmParams / GemmParamsSoft / GemmParamsPen, DecAutomata / DecSoftAutomata /
// DecPenAutomata, BeamAutomata / BeamSoftAutomata) have no one kernel-pointer type.  Such a family's kernel<I>() is still the
// instantiation itself (raise_lds needs its address), and its `Kernel` is a thunk, Sliced<Launch>: the family's `Launch` holds one
// launch's arguments with the RICHEST trailing struct, and Launch::operator()(kernel) passes them in one line - the call slices
// that struct, by value, to the base the form takes, so every form's argument block is what it is without the richer ones.
template <typename Launch> using Sliced = void (*)(const Launch&);
template <typename Launch, auto K> void sliced_launch(const Launch& l) { l(K); }
template <typename Fam, size_t I> constexpr typename Fam::Kernel form_kernel() {
    constexpr auto k = Fam::template kernel<I>();
    if constexpr (std::is_convertible_v<decltype(k), typename Fam::Kernel>) return k;
    else return sliced_launch<typename Fam::Launch, k>;
}

template <typename Fam, size_t... I> Form<typename Fam::Kernel> find_form(const typename Fam::Args& key, std::index_sequence<I...>) {
    Form<typename Fam::Kernel> r;
    (void)((Fam::forms[I] == key && (r = {form_kernel<Fam, I>(), Fam::lds(Fam::forms[I])}, true)) || ...);
    return r;
}
template <typename Fam> Form<typename Fam::Kernel> find_form(const typename Fam::Args& key) {
    return find_form<Fam>(key, std::make_index_sequence<std::size(Fam::forms)>{});
}
// the row a key names (a family whose rows carry their profile name: operator== leaves the name out); null as find_form's kernel
template <typename Fam> const typename Fam::Args* find_row(const typename Fam::Args& key) {
    const auto it = std::find(std::begin(Fam::forms), std::end(Fam::forms), key);
    return it == std::end(Fam::forms) ? nullptr : &*it;
}

template <typename Fam, size_t... I> void raise_lds(std::index_sequence<I...>) {
    (set_max_lds(Fam::template kernel<I>(), Fam::lds(Fam::forms[I])), ...);
}
template <typename... Fam> void raise_lds() { (raise_lds<Fam>(std::make_index_sequence<std::size(Fam::forms)>{}), ...); }

// ---------------------------------------------------------------------------------------- GEMM
// gemm_kernel (kernels_gemm.h): epilogue x 64 / 128 tiles x two / four ring slots; the two scored masked epilogues also with a
// forced prefix's target column (GemmParams::tgt_val is a template parameter of theirs); the three masked epilogues also in
// their SOFT form (soft token automata: the rows' edge weights go into the tile), on GemmParamsSoft, and in their PEN form
// (repetition penalty), which is SOFT too, on GemmParamsPen - Sliced, so that the plain forms' argument stays GemmParams.
struct TileArgs { int epi, bm, ring; bool tgt, soft, pen; };
constexpr bool operator==(const TileArgs& a, const TileArgs& b) {
    return a.epi == b.epi && a.bm == b.bm && a.ring == b.ring && a.tgt == b.tgt && a.soft == b.soft && a.pen == b.pen;
}
constexpr std::array<TileArgs, 96> tile_forms() {
    std::array<TileArgs, 96> a{};
    int n = 0;
    for (int epi : {EPI_SLAB, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_PATCH, EPI_BIAS_F32, EPI_ARGMAX, EPI_ARGMAX_LSE, EPI_TOPK,
                    EPI_ARGMAX_M, EPI_ARGMAX_LSE_M, EPI_TOPK_M})
        for (int bm : {64, 128})
            for (int ring : {2, 4})
                for (bool tgt : {false, true})
                    for (int rich : {0, 1, 2})      // plain, SOFT, PEN
                        if ((!tgt || epi == EPI_ARGMAX_LSE_M || epi == EPI_TOPK_M) &&
                            (!rich || epi == EPI_ARGMAX_M || epi == EPI_ARGMAX_LSE_M || epi == EPI_TOPK_M))
                            a[n++] = TileArgs{epi, bm, ring, tgt, rich >= 1, rich == 2};
    return a;
}
template <typename T> struct TileFamily {
    using Args = TileArgs;
    struct Launch {
        dim3 grid; int lds; hipStream_t stream; GemmParamsPen p;
        template <typename K> void operator()(K kernel) const { hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, p); }
    };
    using Kernel = Sliced<Launch>;
    static constexpr std::array<Args, 96> forms = tile_forms();
    static_assert(forms[95].bm == 128 && forms[95].tgt && forms[95].pen, "tile_forms fills its table");
    template <size_t I> static constexpr auto kernel() { constexpr Args a = forms[I]; return gemm_kernel<T, a.bm, a.bm, a.epi, a.ring, a.tgt, a.soft, a.pen>; }
    static constexpr int lds(const Args& a) { return a.ring * (a.bm + a.bm) * 128; }
};
// Repetition penalty (the PEN forms): the rows' seen words and penalties (kernels_gemm.h GemmParamsPen)
struct TokPen { const unsigned* seen_mask = nullptr; const float* penalty_of_row = nullptr; };
// Soft token automata (the SOFT forms): the rows' states and the arena's edge tables (kernels_gemm.h GemmParamsSoft)
struct TokSoft { const int* state = nullptr; const int* edge_begin = nullptr; const int* edge_token = nullptr; const float* edge_weight = nullptr; };

// The grid and the ring depth of one gemm_kernel launch: M x N outputs on bm x bm tiles, `split` K slices of `ktiles` K-tiles
// each, `ybatch` GEMMs (heads).  launch_gemm_tile launches what this says and decode_plan reports it (mocr_decode_plan: "ring
// slots"), so the rule below is stated once.
struct TileLaunch { int ntm, ntn; long long blocks; int ring; };
struct LastTile { int bm, ring, blocks, split; };
static thread_local LastTile g_last_tile{};      // what this thread's last launch_gemm_tile launched (mocr_op_gemm_args reports it)
static TileLaunch tile_launch(const mocr_engine* e, int M, int N, int bm, int split, int ybatch, int ktiles) {
    TileLaunch t{};
    t.ntn = N / bm; t.ntm = (M + bm - 1) / bm;
    t.blocks = (long long)t.ntm * t.ntn * ybatch * split;
    // Grids of at most one block per CU walk their K-tiles alone on a CU, one memory round trip per K-tile on the two-slot
    // ring.  A four-slot ring (three K-tiles in flight, 128 KiB of LDS for the 128 x 128 tile) changed nothing for the encoder
    // of a few crops (r02: QKV of one crop 16.1 vs 15.9 us - its cost is the DMA issue), but the decode step's split-K
    // projections of a batch decoding ALONE are such grids too (240 blocks x 6-24 K-tiles at 2560 rows): r04,
    // tools/r04_deep_ab.sh, isolated batches, two / four slots: 128 rows 68.0 / 66.2 ms, 256 rows 90.6 / 88.6, 320 rows 108.5 /
    // 104.7, 512 rows 128.5 / 122.4, 1024 rows 196.0 / 193.7 - and the headline's two lanes x 2560 rows 7.02-7.11 / 6.90-6.92 k
    // crops/s: two 64-KiB blocks of two lanes share a CU, a 128-KiB block does not.  So: four slots for batches below the
    // rows from which a queue is split over two lanes (1280).  Same K order, same sums: bit-identical either way.
    // The rule, as the plan reports it: four slots iff M < 1280 rows, at least 4 K-tiles per K slice and at most one block per
    // CU in the whole grid (N-tiles x M-tiles x heads x K slices); two slots otherwise.
    static const int deep_rows = env_int("MOCR_GEMM_DEEP_ROWS", 1280);
    static const int deep_mult64 = env_int("MOCR_GEMM_DEEP_MULT64", 1);      // (experiments: 64 x 64 tiles, two 64-KiB rings fit a CU)
    // (the ring depth does not touch the arithmetic, so a compacted batch's tail chooses it by the rows it has LEFT, as
    // launch_qqt its rows per block: r04, tools/r04_neutral_ab.sh, mixed-lengths leg 11.93 -> 12.11 k crops/s, ids bit-identical;
    // MOCR_NEUTRAL_BY_ROWS=0: by the batch's regime)
    static const int neutral_by_rows = env_int("MOCR_NEUTRAL_BY_ROWS", 2);
    const bool deep = (neutral_by_rows ? M : e->rrows(M)) < deep_rows && ktiles >= 4 &&
                      t.blocks <= (long long)e->num_cus * (bm == 64 ? deep_mult64 : 1);
    t.ring = deep ? 4 : 2;
    return t;
}

template <typename T>
void launch_gemm_tile(mocr_engine* e, const GemmParams& p0, int epi, int bm, int split, int ybatch, const TokSoft* soft = nullptr,
                      const TokPen* pen = nullptr) {
    GemmParamsPen p{};      // the richest argument: a form takes the base it is declared with (TileFamily::Launch)
    static_cast<GemmParams&>(p) = p0;
    const TileLaunch t = tile_launch(e, p.M, p.N, bm, split, ybatch, p.k_per_split / (128 / (int)sizeof(T)));
    p.ntn = t.ntn; p.ntm = t.ntm;
    if (soft) { p.aut_state = soft->state; p.edge_begin = soft->edge_begin; p.edge_token = soft->edge_token; p.edge_weight = soft->edge_weight; }
    if (pen) { p.seen_mask = pen->seen_mask; p.penalty_of_row = pen->penalty_of_row; }
    // (a penalty's form is a SOFT one whether or not `soft` is given: a penalty without any automaton)
    const TileArgs key{epi, bm, t.ring, p.tgt_val != nullptr, soft || pen, pen != nullptr};
    const auto f = find_form<TileFamily<T>>(key);
    if (!f.kernel)
        throw ArgError{key.pen ? "a repetition penalty goes into the masked LM-head epilogues"
                               : key.soft ? "edge weights go into the masked LM-head epilogues" : "unknown GEMM epilogue", MOCR_ERR_ARG};
    f.kernel({dim3(p.ntm * p.ntn, ybatch, split), f.lds, e->stream, p});
    HIPCHECK(hipGetLastError());
    g_last_tile = {bm, t.ring, (int)std::min<long long>(t.blocks, INT32_MAX), split};
}

#ifdef MOCR_EXPERIMENTS
// The A/B kernels of kernels_gemm_lab.h: gemm256_kernel, gemm_wide_kernel (256 x 128 / 256 x 256 tiles: WN = 2 / 4), gemm_wide2_kernel.
struct EpiArgs { int epi, wn; };      // (wn: gemm_wide_kernel only)
constexpr bool operator==(const EpiArgs& a, const EpiArgs& b) { return a.epi == b.epi && a.wn == b.wn; }
struct Gemm256Family {
    using Args = EpiArgs;
    using Kernel = void (*)(GemmParams);
    static constexpr Args forms[] = {{EPI_BIAS, 0}, {EPI_BIAS_GELU, 0}, {EPI_BIAS_RESID, 0}, {EPI_PATCH, 0}, {EPI_BIAS_F32, 0}};
    template <size_t I> static constexpr Kernel kernel() { return gemm256_kernel<forms[I].epi>; }
    static constexpr int lds(const Args&) { return 3 * (256 + 128) * 128; }
};
struct WideFamily {
    using Args = EpiArgs;
    using Kernel = void (*)(GemmParams);
    static constexpr Args forms[] = {{EPI_BIAS, 2}, {EPI_BIAS_GELU, 2}, {EPI_BIAS_RESID, 2}, {EPI_BIAS, 4}, {EPI_BIAS_GELU, 4}, {EPI_BIAS_RESID, 4}};
    template <size_t I> static constexpr Kernel kernel() { return gemm_wide_kernel<forms[I].epi, forms[I].wn>; }
    static constexpr int lds(const Args& a) { return 3 * (256 + 64 * a.wn) * 64; }
};
struct Wide2Family {
    using Args = EpiArgs;
    using Kernel = void (*)(GemmParams);
    static constexpr Args forms[] = {{EPI_BIAS, 0}, {EPI_BIAS_GELU, 0}, {EPI_BIAS_RESID, 0}};
    template <size_t I> static constexpr Kernel kernel() { return gemm_wide2_kernel<forms[I].epi>; }
    static constexpr int lds(const Args&) { return 4 * (256 + 256) * 64; }
};

void launch_gemm256(mocr_engine* e, const GemmParams& p0, int epi) {
    const auto f = find_form<Gemm256Family>({epi, 0});
    if (!f.kernel) throw ArgError{"gemm256: unsupported epilogue", MOCR_ERR_ARG};
    GemmParams p = p0;
    p.ntn = p.N / 128; p.ntm = (p.M + 255) / 256;
    hipLaunchKernelGGL(f.kernel, dim3(p.ntm * p.ntn), dim3(256), f.lds, e->stream, p);
    HIPCHECK(hipGetLastError());
}

// one tile per block; the grid is rounded up to 8 so that every XCD gets the same count (an empty block returns at once)
void launch_gemm_wide(mocr_engine* e, const GemmParams& p0, int epi, int wn) {
    const auto f = find_form<WideFamily>({epi, wn});
    if (!f.kernel) throw ArgError{"wide gemm: unsupported epilogue", MOCR_ERR_ARG};
    GemmParams p = p0;
    p.ntn = p.N / (64 * wn); p.ntm = (p.M + 255) / 256;
    hipLaunchKernelGGL(f.kernel, dim3((p.ntm * p.ntn + 7) / 8 * 8), dim3(128 * wn), f.lds, e->stream, p);
    HIPCHECK(hipGetLastError());
}

void launch_gemm_wide2(mocr_engine* e, const GemmParams& p0, int epi) {
    if (p0.k_per_split % 64 || p0.k_per_split < 128) throw ArgError{"wide2 gemm: K must be a multiple of 64, >= 128", MOCR_ERR_ARG};
    const auto f = find_form<Wide2Family>({epi, 0});
    if (!f.kernel) throw ArgError{"wide2 gemm: unsupported epilogue", MOCR_ERR_ARG};
    GemmParams p = p0;
    p.ntn = p.N / 256; p.ntm = (p.M + 255) / 256;
    static const int stagger_env = env_int("MOCR_GEMM_STAGGER", -1);
    p.stagger = stagger_env > 0 ? stagger_env : 0;      // measured r02: no gain (the store drain is not what a phase shift hides), default off
    p.first_round = e->num_cus;
    hipLaunchKernelGGL(f.kernel, dim3((p.ntm * p.ntn + 7) / 8 * 8), dim3(512), f.lds, e->stream, p);
    HIPCHECK(hipGetLastError());
}
#endif  // MOCR_EXPERIMENTS

// The strip schedule of the persistent kernel (kernels_gemm_pers.h, STRIP): rows per strip for a grid of `grid` blocks,
// 0 when the grid cannot hold a strip.  Host mirror of the kernel's arithmetic.
static int pers_strip_rows(int M, int ntn, int grid) {
    const int slots = grid >> 3, spx = slots / ntn;
    const int nstrips = 8 * spx + (8 * (slots - spx * ntn)) / ntn;
    if (nstrips <= 0) return 0;
    const int U = (M + 15) >> 4;
    return ((U + nstrips - 1) / nstrips) * 16;
}

// Rounds of 256 x 256 tiles the slowest block walks: tile list (XCD chunks dealt round-robin) vs strips (a half tile costs
// ~0.6 of a tile: one wave per SIMD multiplies).
static bool pers_strip_wins(int M, int ntn, int grid) {
    const int ntiles = ((M + 255) / 256) * ntn;
    if (ntiles < 2 * grid) return false;
    const int chunk = (ntiles + 7) / 8, per_block = (chunk + (grid >> 3) - 1) / (grid >> 3);
    const int R = pers_strip_rows(M, ntn, grid);
    if (!R) return false;
    const int rem = R & 255;
    // (a half tile: 0.5-0.75 of a tile by its K; FC1 at batch 256 - 9 tiles + a half tile against 10 - measured 274-279 ->
    // 265-271 us with the 64-deep image)
    const double strip_cost = (R >> 8) + (rem == 0 ? 0.0 : rem <= 128 ? 0.6 : 1.0);
    return strip_cost <= 0.965 * per_block;
}

// gemm_pers_kernel (kernels_gemm_pers.h): <epilogue, split DMA, pair loop, strips, LayerNorm fold>.  The product runs split DMA
// on the one-barrier-per-two-K-tiles loop (K64: 64-deep LDS image, whole-line DMA requests), every epilogue with and without
// strips and fold.
struct PersArgs { int epi; bool split_dma, pair, strip, lnf; };
constexpr bool operator==(const PersArgs& a, const PersArgs& b) {
    return a.epi == b.epi && a.split_dma == b.split_dma && a.pair == b.pair && a.strip == b.strip && a.lnf == b.lnf;
}
struct PersFamily {
    using Args = PersArgs;
    using Kernel = void (*)(GemmParams);
    static constexpr Args forms[] = {
        {EPI_BIAS, true, true, false, false}, {EPI_BIAS, true, true, true, false}, {EPI_BIAS, true, true, false, true}, {EPI_BIAS, true, true, true, true},
        {EPI_BIAS_GELU, true, true, false, false}, {EPI_BIAS_GELU, true, true, true, false}, {EPI_BIAS_GELU, true, true, false, true}, {EPI_BIAS_GELU, true, true, true, true},
        {EPI_BIAS_RESID, true, true, false, false}, {EPI_BIAS_RESID, true, true, true, false}, {EPI_BIAS_RESID, true, true, false, true}, {EPI_BIAS_RESID, true, true, true, true},
#ifdef MOCR_EXPERIMENTS
        // the one-barrier-per-K-tile loop on the 32-deep image, A/B partner of the pair loop (its fp32-residual form never folds)
        {EPI_BIAS, true, false, false, false}, {EPI_BIAS, true, false, true, false}, {EPI_BIAS, true, false, false, true}, {EPI_BIAS, true, false, true, true},
        {EPI_BIAS_GELU, true, false, false, false}, {EPI_BIAS_GELU, true, false, true, false}, {EPI_BIAS_GELU, true, false, false, true}, {EPI_BIAS_GELU, true, false, true, true},
        {EPI_BIAS_RESID, true, false, false, false}, {EPI_BIAS_RESID, true, false, true, false},
        // every wave requests LDS-DMA: both loops, tile list only
        {EPI_BIAS, false, false, false, false}, {EPI_BIAS_GELU, false, false, false, false}, {EPI_BIAS_RESID, false, false, false, false},
        {EPI_BIAS, false, true, false, false}, {EPI_BIAS_GELU, false, true, false, false}, {EPI_BIAS_RESID, false, true, false, false},
#endif
    };
    template <size_t I> static constexpr Kernel kernel() { constexpr Args a = forms[I]; return gemm_pers_kernel<a.epi, a.split_dma, a.pair, a.strip, a.lnf>; }
    static constexpr int lds(const Args&) { return PERS_LDS; }
};

// What this thread's last launch_gemm_pers launched (mocr_last_pers_launch reports it)
struct LastPers { int blocks, strips, tiles, group_n; };
static thread_local LastPers g_last_pers{};

// One launch of the persistent kernel.  blocks = 0: one block per CU (a multiple of 8, at most one per tile); a test may ask for
// fewer blocks (longer tile sequences).  strip: 0 tile list, 1 strips wherever the grid can hold one, -1 whichever walks fewer
// rounds; strips exist for the split-DMA forms only.  p.ln_part set: the LayerNorm-folding forms (kernels_gemm_pers.h, LNF).
void launch_gemm_pers(mocr_engine* e, const GemmParams& p0, int epi, bool split_dma, bool pair, int blocks, int strip) {
    GemmParams p = p0;
    if (p.k_per_split % 64 || p.k_per_split < 128) throw ArgError{"persistent gemm: K must be a multiple of 64, >= 128", MOCR_ERR_ARG};
    const bool lnf = p.ln_part != nullptr;
    if (lnf && !(split_dma && (epi == EPI_BIAS_RESID ? (pair && p.N <= 1024 && p.xb) : p.csum != nullptr)))
        throw ArgError{"persistent gemm: LayerNorm folding needs the product kernel forms and their operands", MOCR_ERR_ARG};
    p.ntn = p.N / 256; p.ntm = (p.M + 255) / 256;
    const int grid = std::max(8, std::min(blocks > 0 ? blocks : e->num_cus, (p.ntm * p.ntn + 7) / 8 * 8) / 8 * 8);
    const bool strips = split_dma && strip && (strip > 0 ? pers_strip_rows(p.M, p.ntn, grid) > 0 : pers_strip_wins(p.M, p.ntn, grid));
    // (a strip's tile reads a whole 256-row window of A that ends with the tile's last row: below 256 rows it would start above A)
    if (strips && p.M < 256) throw ArgError{"persistent gemm: the strip schedule needs at least 256 rows", MOCR_ERR_ARG};
    const auto f = find_form<PersFamily>({epi, split_dma, pair, strips, lnf});
    if (!f.kernel && lnf) throw ArgError{"persistent gemm: no LayerNorm-folding form of this kernel variant", MOCR_ERR_ARG};
    if (!f.kernel) throw ArgError{"persistent gemm: unsupported epilogue", MOCR_ERR_ARG};
    static const int stagger_env = env_int("MOCR_GEMM_STAGGER", 0);
    p.stagger = stagger_env;
    static const int hpos_env = env_int("MOCR_GEMM_HPOS", 0);
    p.first_round = hpos_env;
    hipLaunchKernelGGL(f.kernel, dim3(grid), dim3(512), f.lds, e->stream, p);
    HIPCHECK(hipGetLastError());
    g_last_pers = {grid, strips ? 1 : 0, p.ntm * p.ntn, p.group_n};
}

// Tile codes.  The numbers belong to the boundaries that own them (mocr_op_gemm / mocr_op_gemm_ln, the MOCR_*_TILE knobs, DESIGN's
// appendix, the tests); inside, this one table says what a code means and everybody else asks the row.
enum class GemmKind { Tile, Persistent, Lab256, Wide, Wide2, LabOnly };
struct TileCode {
    int code;
    GemmKind kind;
    int arg;                  // Tile: the tile's rows = columns; Wide: WN
    int blocks;               // Persistent: 0 = one block per CU, 8 = a test hook, 8 blocks walk all the tiles
    int strip;                // Persistent: 0 tile list, 1 the strip schedule forced (test hooks), -1 by the shape (MOCR_GEMM_STRIP)
    bool split_dma, pair;     // Persistent: the kernel form (PersArgs)
    bool knobs;               // Persistent: the codes of the product, which MOCR_GEMM_PAIR_BF16 moves to the other loop
    bool persistent() const { return kind == GemmKind::Persistent; }
    bool product_persistent() const { return persistent() && knobs && !blocks && strip < 0; }      // the form run_encoder picks (and folds)
};
constexpr int TILE_PERSISTENT = 4096;
constexpr TileCode TILE_CODES[] = {
    {64, GemmKind::Tile, 64}, {128, GemmKind::Tile, 128},
    // one barrier per two K-tiles for the fp32-residual GEMMs (r03, M = 50,432: O-proj 137 -> 129 us, FC2 305 -> 302; the
    // bf16-output GEMMs lose with it: QKV 175 -> 208 us)
    // 4097: a test hook, 8 blocks walk all the tiles; 4099 / 4100: the strip schedule forced (whole grid / 8 blocks) - test hooks too
    {TILE_PERSISTENT, GemmKind::Persistent, 0, 0, -1, true, true, true}, {4097, GemmKind::Persistent, 0, 8, 0, true, true, true},
    {4099, GemmKind::Persistent, 0, 0, 1, true, true, true}, {4100, GemmKind::Persistent, 0, 8, 1, true, true, true},
#ifdef MOCR_EXPERIMENTS
    {256, GemmKind::Lab256}, {512, GemmKind::Wide, 2}, {1024, GemmKind::Wide, 4}, {2048, GemmKind::Wide2},
    {4098, GemmKind::Persistent, 0, 0, 0, false, false},                                                        // every wave requests LDS-DMA
    {4101, GemmKind::Persistent, 0, 0, 0, true, true}, {4102, GemmKind::Persistent, 0, 8, 0, true, true},      // one barrier per two K-tiles
    {4103, GemmKind::Persistent, 0, 0, 1, true, false}, {4104, GemmKind::Persistent, 0, 8, 1, true, false},    // strips on the one-barrier-per-K-tile loop
    {4105, GemmKind::Persistent, 0, 0, 0, false, true}, {4106, GemmKind::Persistent, 0, 8, 0, false, true},    // the pair loop with every wave requesting LDS-DMA
#else
    {256, GemmKind::LabOnly}, {512, GemmKind::LabOnly}, {1024, GemmKind::LabOnly}, {2048, GemmKind::LabOnly}, {4098, GemmKind::LabOnly},
#endif
};
static const TileCode* tile_code(int code) {
    for (const TileCode& t : TILE_CODES) if (t.code == code) return &t;
    return nullptr;      // not a tile code
}
static bool tile_is(int code, GemmKind kind) { const TileCode* t = tile_code(code); return t && t->kind == kind; }

struct HeadBatch { int heads = 1; long long a_yoff = 0, w_yoff = 0, o_yoff = 0, b_yoff = 0; int ldw = 0; };
// LayerNorm folded into the persistent encoder GEMMs (tile code 4096; kernels_gemm_pers.h LNF).  EPI_BIAS_RESID: `part` and
// `xb` are written; EPI_BIAS / EPI_BIAS_GELU: `part` and `csum` are read (W and bias are the folded ones).
struct LnFold { float* part = nullptr; const float* csum = nullptr; void* xb = nullptr; };
// Token constraints (EPI_*_M): the set table, the set of every batch row and the slot -> row map (kernels_gemm.h GemmParams)
struct TokMask { const unsigned* table = nullptr; const int* set_of_row = nullptr; const int* rowmap = nullptr; };
// What the fused LM-head epilogues write per N-tile beside the candidate values in `out`: the columns (every EPI_ARGMAX* /
// EPI_TOPK*), the exp sums (the _LSE and TOPK forms), the four best (TOPK) - and the mask the EPI_*_M forms apply
// Forced prefixes (EPI_ARGMAX_LSE_M / EPI_TOPK_M): the rows' prefixes, the slots' steps and where the target column's value goes
struct TokTarget { const int* prefix = nullptr; const int* prefix_len = nullptr; int prefix_ld = 0; const int* step = nullptr; float* tgt_val = nullptr; };
struct LmHead { int* cand_idx = nullptr; float* cand_sum = nullptr; float* top_val = nullptr; int* top_idx = nullptr; TokMask mask; TokTarget target; TokSoft soft; TokPen pen; };

// One GEMM: A [M,K] (lda), W [N,K] (ldw = K), out (ldo).  tile: a tile code (TILE_CODES).  gemm_call states the operands and the
// shape; a call site then names every extra it sets.  split > 1 only with EPI_SLAB.
struct GemmCall {
    const char* name;
    const void* A; int lda;
    const void* W; const float* bias;
    void* out; int ldo;
    int M, N, K, epi, tile;
    const float* resid = nullptr;                       // EPI_BIAS_RESID
    int split = 1; long long slab_stride = 0;           // EPI_SLAB: K slices, and the elements between two slices' slabs
    const float* pos = nullptr; int patches = 0;        // EPI_PATCH: the position table and the patches per crop
    const HeadBatch* hb = nullptr;                      // one GEMM per head (grid.y)
    int group_n = 0;                                    // N-tiles per column group of the tile order (0: none)
    const LmHead* lm = nullptr;                         // the fused LM-head epilogues
    const LnFold* lnf = nullptr;                        // LayerNorm folded in
};
static GemmCall gemm_call(const char* name, const void* A, int lda, const void* W, const float* bias, void* out, int ldo, int M, int N,
                          int K, int epi, int tile) {
    GemmCall c{};
    c.name = name; c.A = A; c.lda = lda; c.W = W; c.bias = bias; c.out = out; c.ldo = ldo; c.M = M; c.N = N; c.K = K; c.epi = epi; c.tile = tile;
    return c;
}

#ifdef MOCR_EXPERIMENTS
// Diagnostics of the persistent kernel, MOCR_GEMM_ABLATE & 8192 (kernels_gemm_pers.h, MOCR_STAMP): the kernel's cycle stamps go
// to a buffer passed in GemmParams::pos (stamps_arm) and are summed up per role behind the launch (stamps_report).
static unsigned long long* g_stamp_buf = nullptr;
static void stamps_arm(mocr_engine* e, GemmParams& p) {
    if (!g_stamp_buf) HIPCHECK(hipMalloc(&g_stamp_buf, 1024 * 8 * 4 * 8));
    HIPCHECK(hipMemsetAsync(g_stamp_buf, 0, 1024 * 8 * 4 * 8, e->stream));
    p.pos = reinterpret_cast<const float*>(g_stamp_buf);
}
static void stamps_report(mocr_engine* e, const char* name) {
    if (!g_stamp_buf) return;
    HIPCHECK(hipStreamSynchronize(e->stream));
    std::vector<unsigned long long> h(256 * 8 * 4);
    HIPCHECK(hipMemcpy(h.data(), g_stamp_buf, h.size() * 8, hipMemcpyDeviceToHost));
    double s0[2] = {0, 0}, s1[2] = {0, 0}, s2[2] = {0, 0}, pairs = 0;
    int nb = 0;
    for (int b = 0; b < 256; ++b) {
        if (!h[(b * 8) * 4 + 3]) continue;
        ++nb;
        pairs += (double)h[(b * 8) * 4 + 3] / 2;
        for (int w = 0; w < 8; ++w) { s0[w >> 2] += h[(b * 8 + w) * 4]; s1[w >> 2] += h[(b * 8 + w) * 4 + 1]; s2[w >> 2] += h[(b * 8 + w) * 4 + 2]; }
    }
    if (nb) {
        const double n = pairs * 4;      // wave-pairs per role
        fprintf(stderr, "[stamps] %s: %d blocks, %.0f K-tile pairs each; cycles per pair  DMA waves: work %.0f, DMA wait %.0f, barrier %.0f | store waves: work %.0f, -, barrier %.0f\n",
                name, nb, pairs / nb, s0[0] / n, s1[0] / n, s2[0] / n, s0[1] / n, (s1[1] + s2[1]) / n);
    }
}
#endif

template <typename T>
void gemm(mocr_engine* e, const GemmCall& c) {
    const int M = c.M, N = c.N, K = c.K, epi = c.epi, tile = c.tile, split = c.split;
    const LmHead* const lm = c.lm;
    const int kt = 128 / (int)sizeof(T);
    if (N % (tile >= 1024 ? 256 : tile >= 256 ? 128 : std::max(tile, 1)) || K % (kt * split) || (split > 1 && epi != EPI_SLAB) ||
        (tile >= 256 && (sizeof(T) != 2 || split != 1)))
        throw ArgError{std::string("gemm shape not tileable: ") + c.name, MOCR_ERR_ARG};
    GemmParams p{};
    p.A = c.A; p.W = c.W; p.bias = c.bias; p.out = c.out; p.resid = c.resid; p.pos = c.pos;
    const TokMask tm = lm ? lm->mask : TokMask{};
    if ((epi == EPI_ARGMAX_M || epi == EPI_ARGMAX_LSE_M || epi == EPI_TOPK_M) != (tm.table || tm.set_of_row) || !tm.table != !tm.set_of_row)
        throw ArgError{std::string("the masked LM-head epilogues come with a token-set table: ") + c.name, MOCR_ERR_ARG};
    if (lm) {
        p.cand_idx = lm->cand_idx; p.cand_sum = lm->cand_sum; p.top_val = lm->top_val; p.top_idx = lm->top_idx;
        if (tm.table) { p.tok_mask = tm.table; p.set_of_row = tm.set_of_row; p.rowmap = tm.rowmap; }
        const TokTarget& tt = lm->target;
        if (tt.tgt_val) {
            if ((epi != EPI_ARGMAX_LSE_M && epi != EPI_TOPK_M) || !tt.prefix || !tt.prefix_len || !tt.step || tt.prefix_ld < 1)
                throw ArgError{std::string("a target column comes with the masked, scored LM-head epilogues and all five arrays: ") + c.name, MOCR_ERR_ARG};
            p.prefix = tt.prefix; p.prefix_len = tt.prefix_len; p.prefix_ld = tt.prefix_ld; p.step = tt.step; p.tgt_val = tt.tgt_val;
        }
    }
    const TokSoft* const soft = lm && lm->soft.state ? &lm->soft : nullptr;
    if (soft && (!tm.table || !soft->edge_begin || !soft->edge_token || !soft->edge_weight || !tile_is(tile, GemmKind::Tile)))
        throw ArgError{std::string("edge weights come with a masked LM-head epilogue on a 64 / 128 tile and all four arrays: ") + c.name, MOCR_ERR_ARG};
    const TokPen* const pen = lm && lm->pen.seen_mask ? &lm->pen : nullptr;
    if (pen && (!tm.table || !pen->penalty_of_row || !tile_is(tile, GemmKind::Tile)))
        throw ArgError{std::string("a repetition penalty comes with a masked LM-head epilogue on a 64 / 128 tile and both arrays: ") + c.name, MOCR_ERR_ARG};
    p.M = M; p.N = N; p.lda = c.lda; p.ldw = K; p.ldo = c.ldo;
    int ybatch = 1;
    if (const HeadBatch* hb = c.hb) {
        if (epi != EPI_BIAS || tile >= 256) throw ArgError{"per-head batched GEMM needs EPI_BIAS on the 64/128 kernel", MOCR_ERR_ARG};
        ybatch = hb->heads; p.a_yoff = hb->a_yoff; p.w_yoff = hb->w_yoff; p.o_yoff = hb->o_yoff; p.b_yoff = hb->b_yoff;
        if (hb->ldw) p.ldw = hb->ldw;
    }
    p.k_per_split = K / split; p.slab_stride = c.slab_stride; p.patches = c.patches;
    if (c.lnf) {
        if (tile < 4096 || tile > 4100 || sizeof(T) != 2) throw ArgError{"LayerNorm folding: persistent bf16 GEMMs only", MOCR_ERR_ARG};
        p.ln_part = c.lnf->part; p.csum = c.lnf->csum; p.xb = c.lnf->xb; p.ln_eps = e->cfg.ln_eps;
    }
    const TileCode* const tc = tile_code(tile);
    static const int ablate = env_int("MOCR_GEMM_ABLATE", 0);
    p.ablate = ablate;
#ifdef MOCR_EXPERIMENTS
    const bool stamps = (ablate & 8192) && tc && tc->persistent();
    if (stamps && epi != EPI_PATCH) stamps_arm(e, p);
#endif
    static const int group_env = env_int("MOCR_GEMM_GROUPN", -1);
    p.group_n = group_env >= 0 ? group_env : c.group_n;
    const double out_b = (epi == EPI_BIAS || epi == EPI_BIAS_GELU) ? sizeof(T) : 4.0;
    const double bytes = ((double)M * K + (double)N * K) * sizeof(T) + (double)M * N * out_b * (epi == EPI_SLAB ? split : 1) +
                         (epi == EPI_BIAS_RESID ? (double)M * N * 4 : 0) + (c.lnf && epi == EPI_BIAS_RESID ? (double)M * N * 2 : 0);
    ProfScope ps(e, c.name, 2.0 * M * N * K * ybatch, bytes * ybatch);
    if (!tc) throw ArgError{"gemm tile must be 64, 128 or 4096", MOCR_ERR_ARG};
    switch (tc->kind) {
        case GemmKind::Tile: launch_gemm_tile<T>(e, p, epi, tc->arg, split, ybatch, soft, pen); break;
        case GemmKind::Persistent: {
            static const int strip_env = env_int("MOCR_GEMM_STRIP", -1);     // -1: strips where they walk fewer rounds (r03, M = 50,432: O-proj 133 -> 113 us, FC2 303 -> 275)
            // the bf16-epilogue GEMMs: 1 = the one-barrier-per-two-K-tiles loop with the 64-deep LDS image (K64), 0 = one barrier per
            // 32-deep K-tile, three K-tiles in flight (r03 first session's choice, when both loops fed on half-line requests)
            static const int pair_bf16 = env_int("MOCR_GEMM_PAIR_BF16", 1);
            const bool pair = tc->pair && !(tc->knobs && epi != EPI_BIAS_RESID && !pair_bf16);
            launch_gemm_pers(e, p, epi, tc->split_dma, pair, tc->blocks, tc->strip < 0 ? strip_env : tc->strip);
            break;
        }
#ifdef MOCR_EXPERIMENTS
        case GemmKind::Lab256: launch_gemm256(e, p, epi); break;
        case GemmKind::Wide: launch_gemm_wide(e, p, epi, tc->arg); break;
        case GemmKind::Wide2: launch_gemm_wide2(e, p, epi); break;
#endif
        default: throw ArgError{"this GEMM tile code is an A/B kernel of the experiments build (build.py --experiments)", MOCR_ERR_UNSUPPORTED};
    }
#ifdef MOCR_EXPERIMENTS
    if (stamps) stamps_report(e, c.name);
#endif
}

// ---------------------------------------------------------------------------------------- encoder
template <typename T>
void layernorm(mocr_engine* e, const float* x, const float* g, const float* b, void* out, int M) {
    ProfScope ps(e, "layernorm", 0, (double)M * e->D * (4 + sizeof(T)));
    hipLaunchKernelGGL((layernorm_kernel<T, 768>), dim3((M + 3) / 4), dim3(256), 0, e->stream, x, g, b,
                       reinterpret_cast<T*>(out), M, e->cfg.ln_eps);
    HIPCHECK(hipGetLastError());
}

// The encoder attentions: four kernels with argument lists of their own, so their family is the list of (kernel, LDS) that
// init_kernel_attrs walks; enc_attention launches each with the same constant.
constexpr int ENC_SIMPLE_LDS = (200 * 65 + 200 * 64 + 4 * 64 + 4 * 256) * 4;
#ifdef MOCR_EXPERIMENTS
constexpr int ENC_MFMA_R02_LDS = ENC_SP * 128 + 64 * ENC_VT_LD * 2;
#endif
template <typename T, typename F> void for_each_enc_attn(F&& f) {
    f(enc_attn_simple_kernel<T>, ENC_SIMPLE_LDS);
    f(enc_attn2_kernel, EA2_LDS);
    f(enc_attn_f32_kernel, EAF_LDS);
#ifdef MOCR_EXPERIMENTS
    f(enc_attn_mfma_kernel, ENC_MFMA_R02_LDS);
#endif
}

// Blocks per (image, head) of the encoder attention of n crops: only enc_attn2_kernel (bf16, impl 1) shares a head among blocks.
// A few crops: two / four blocks per (image, head) share its thirteen 16-query units while n * H blocks would leave most of
// the chip idle (three blocks fit a CU).  On 256 CUs: up to 10 crops four blocks, 11 .. 21 two, from 22 one.
template <typename T>
int enc_attn_ysplit(const mocr_engine* e, int n, int impl) {
    if (impl != 1 || sizeof(T) != 2) return 1;
    const long long blocks = (long long)n * e->H;
    return blocks * 4 <= 2LL * e->num_cus ? 4 : blocks * 2 <= 2LL * e->num_cus ? 2 : 1;
}

// (ysplit: enc_attn_ysplit's answer - the encoder passes its plan's)
template <typename T>
void enc_attention(mocr_engine* e, const void* qkv, void* ctx, int n, int impl, int ysplit) {
    const int S = e->S, H = e->H;
    const double flops = 4.0 * n * H * (double)S * S * 64;
    const double bytes = (double)n * S * e->D * 4 * sizeof(T);
    if (impl == 1 && sizeof(T) == 2) {
        ProfScope ps(e, "enc_attn_mfma", flops, bytes);
        static const int ablate2_env = env_int("MOCR_ENC_ATTN_ABLATE", 0);
        hipLaunchKernelGGL(enc_attn2_kernel, dim3(n * H, ysplit), dim3(256), EA2_LDS, e->stream,
                           reinterpret_cast<const bf16_t*>(qkv), reinterpret_cast<bf16_t*>(ctx), H, 3 * e->D, e->D, ablate2_env);
#ifdef MOCR_EXPERIMENTS
    } else if (impl == 2 && sizeof(T) == 2) {          // r01-r02 kernel (K / V staged through registers), A/B only
        ProfScope ps(e, "enc_attn_mfma_r02", flops, bytes);
        static const int qsplit_env = env_int("MOCR_ENC_ATTN_QSPLIT", 1);
        const int qsplit = (qsplit_env && n * H * 2 <= e->num_cus) ? 2 : 1;
        static const int ablate_env = env_int("MOCR_ENC_ATTN_ABLATE", 0);
        hipLaunchKernelGGL(enc_attn_mfma_kernel, dim3(n * H, qsplit), dim3(256), ENC_MFMA_R02_LDS, e->stream,
                           reinterpret_cast<const bf16_t*>(qkv), reinterpret_cast<bf16_t*>(ctx), H, 3 * e->D, e->D, ablate_env);
#endif
    } else if (impl == 1 && sizeof(T) == 4) {          // r04: the parity mode on the f32-input matrix cores
        ProfScope ps(e, "enc_attn_f32_mfma", flops, bytes);
        hipLaunchKernelGGL(enc_attn_f32_kernel, dim3(n * H), dim3(256), EAF_LDS, e->stream, reinterpret_cast<const float*>(qkv),
                           reinterpret_cast<float*>(ctx), H, 3 * e->D, e->D);
    } else {
        ProfScope ps(e, "enc_attn_simple", flops, bytes);
        hipLaunchKernelGGL((enc_attn_simple_kernel<T>), dim3(n * H), dim3(256), ENC_SIMPLE_LDS, e->stream,
                           reinterpret_cast<const T*>(qkv), reinterpret_cast<T*>(ctx), S, H, 3 * e->D, e->D, 0.125f);
    }
    HIPCHECK(hipGetLastError());
}

// calibrate_ln_fold's observer: X [M, 768] is the input of the LayerNorm about to run.  Per row, the rounding noise the GEMM
// behind it sees when it is fed bf16(x) (the fold) over the noise when it is fed bf16(LN(x)) (the launch):
//     sqrt( sum_k (x_k g_k rstd)^2 / sum_k ((x_k - mean) rstd g_k + b_k)^2 ),    rms over the rows; the worst LayerNorm counts.
static void calib_observe(mocr_engine* e, int M) {
    auto& c = *e->calib;
    if (c.idx >= c.g.size()) return;                 // (the encoder's final LayerNorm is never folded)
    const int D = e->D;
    c.hx.resize((size_t)M * D);
    HIPCHECK(hipMemcpyAsync(c.hx.data(), e->X, (size_t)M * D * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    const std::vector<float>&g = c.g[c.idx], &b = c.b[c.idx];
    double num = 0.0, den = 0.0;
    for (int m = 0; m < M; ++m) {
        const float* x = c.hx.data() + (size_t)m * D;
        double s = 0.0, q = 0.0;
        for (int k = 0; k < D; ++k) s += x[k];
        const double mean = s / D;
        for (int k = 0; k < D; ++k) { const double d = x[k] - mean; q += d * d; }
        const double rstd = 1.0 / std::sqrt(q / D + (double)e->cfg.ln_eps);
        for (int k = 0; k < D; ++k) {
            const double a = (double)x[k] * g[k] * rstd, y = ((double)x[k] - mean) * rstd * g[k] + b[k];
            num += a * a; den += y * y;
        }
    }
    c.worst = std::max(c.worst, std::sqrt(num / std::max(den, 1e-300)));
    c.idx += 1;
}

// What run_encoder decides from the number of crops (and the engine: its type, its CUs, its slab buffer, its flags) - made
// once, here; run_encoder and the front end consume it and mocr_encoder_plan reports it.
struct EncPlan {
    int embed_tile;                   // patch embedding: 64 / 128
    int tq, to, t1, t2;               // tile codes of QKV / O-proj / FC1 / FC2 (TILE_CODES)
    int split_o, split_2;             // K slices of O-proj / FC2 (1: not split)
    bool fold;                        // the LayerNorms between the layer GEMMs folded into them
    int impl, ysplit;                 // the attention kernel (0 VALU, 1 matrix cores) and its blocks per (image, head)
    int gq, g1;                       // N-tiles per column group of QKV's / FC1's tile order (gemm_tile_of)
};
template <typename T>
EncPlan encoder_plan(const mocr_engine* e, int n) {
    const int D = e->D, F = e->F, M = n * e->S, MPATCH = n * e->G * e->G;
    EncPlan pl{};
    // MOCR_ENC_TILE forces one tile code for the layer GEMMs (experiments); the patch embedding has its own epilogue
    // and stays on the 128x128 kernel unless a tile code that supports it (64/128/256) is forced
    static const int enc_tile_env = env_int("MOCR_ENC_TILE", 0);
    pl.embed_tile = (enc_tile_env && enc_tile_env <= 256) ? enc_tile_env
                    : ((long long)((MPATCH + 127) / 128) * (e->D / 128) * 5 <= 4LL * e->num_cus ? 64 : 128);
    // The 128x128 kernel walks QKV / FC1 in column groups of 9 / 12 N-tiles (a 1.7 / 2.3 MB weight slice stays in
    // the XCD's L2): +4 % / +2 % at M = 806,912 (r01).
    // Layer GEMMs: the 256x256 "wide" kernel (tile code 1024) once it fills the chip about three times over
    // (+12..15 % at M = 806,912, +10..20 % at M = 100,864; even at 12,608 rows), else the 128x128 kernel
    // ... and 64 x 64 tiles while the 128 x 128 grid would leave CUs idle (up to ~0.8 blocks per CU): a block's K-tile costs
    // ~1 us whatever the tile (8 DMA instructions per wave to issue against 32 MFMAs), so a few crops are done sooner as
    // four times as many blocks of a quarter of the work.  r02, encoder of 1 / 4 / 8 crops: 1.41 / 1.49 / 1.54 -> 0.95 /
    // 1.05 / 1.39 ms (QKV of one crop 16.0 -> 10.4 us, O-proj 16.7 -> 9.6, FC1 17.5 -> 11.2, FC2 40.1 -> 21.3)
    auto small_tile = [&](int N) {
        const long long blocks128 = (long long)((M + 127) / 128) * (N / 128);
        return blocks128 * 5 <= 4LL * e->num_cus ? 64 : 128;
    };
    auto layer_tile = [&](int N) {
        if (enc_tile_env) return enc_tile_env;
        const long long tiles = (long long)((M + 255) / 256) * (N / 256);
        // r03: the persistent kernel (tile code 4096, kernels_gemm_pers.h) instead of one 256 x 256 tile per block (2048)
        static const int big_env = env_int("MOCR_ENC_BIG_TILE", 4096);
        // from two tiles per CU (r02 asked for three rounds of one-tile blocks; a persistent block has no turnover to
        // amortise, and at batch 256 the N = 768 GEMMs have 591 tiles)
        // (r03, 64-deep image: from 1.7 tiles per CU - QKV of a 64-crop batch, 441 tiles: 64-68 -> 54 us; MOCR_ENC_BIG_ROUNDS x 10)
        static const int big_rounds10 = env_int("MOCR_ENC_BIG_ROUNDS10", 17);
        // ... and the N = 768 GEMMs also where ONE round of tiles covers half the chip or more (56-111 crops: at 64 crops - 147
        // tiles - FC2 111 -> 96 us and, all four layer GEMMs then being persistent, the LayerNorm launches go: encoder 4.20 ->
        // 3.76 ms; at 128 crops - 297 tiles, two rounds for 1.16 - and at 32 - 75 tiles - the 128 x 128 kernel stays ahead)
        static const int one_round = env_int("MOCR_ENC_ONE_ROUND", 1);
        const bool big = tiles * 10 >= (long long)big_rounds10 * e->num_cus ||
                         (one_round && N <= 1024 && tiles * 2 >= e->num_cus && tiles <= e->num_cus);
        return (sizeof(T) == 2 && big) ? big_env : small_tile(N);
    };
    // per-GEMM overrides for experiments: MOCR_ENC_TILE_QKV / _O / _FC1 / _FC2 (tile codes as in gemm())
    static const int tq_env = env_int("MOCR_ENC_TILE_QKV", 0), to_env = env_int("MOCR_ENC_TILE_O", 0),
                     t1_env = env_int("MOCR_ENC_TILE_FC1", 0), t2_env = env_int("MOCR_ENC_TILE_FC2", 0);
    pl.tq = tq_env ? tq_env : layer_tile(3 * D); pl.to = to_env ? to_env : layer_tile(D); pl.t1 = t1_env ? t1_env : layer_tile(F);
    pl.t2 = t2_env ? t2_env : pl.to;
    // tile order of QKV / FC1: column groups whose weight slices stay in an XCD's 4 MiB L2 while the A row-panels stream through
    // once per group.  128 x 128 tiles: groups of 9 / 12 N-tiles (r01).  Persistent 256 x 256 tiles: groups of 6 (r04: QKV 6 + 3,
    // FC1 6 + 6: the whole 3.4 / 4.5 MiB weight does not fit beside the A panels, and without groups every XCD re-fetches it
    // per round of row-panels - at batch 256 QKV 210 -> 200 us, FC1 337 -> 331 us, one box; tools/r04_groupn_ab.sh)
    pl.gq = tile_is(pl.tq, GemmKind::Persistent) ? 6 : 9;
    pl.g1 = tile_is(pl.t1, GemmKind::Persistent) ? 6 : 12;
    pl.impl = (e->cfg.flags & MOCR_FLAG_SIMPLE_ATTENTION) ? 0 : 1;
    pl.ysplit = enc_attn_ysplit<T>(e, n, pl.impl);
    // A few crops (the 64 x 64 grid of the two N = 768 GEMMs is at most one block per CU: up to 6 crops on 256 CUs): O-proj
    // and FC2 are split over K into fp32 slabs - for one crop 12 / 48 K-tiles walked alone by 48 blocks become 4 / 6 K-tiles
    // on 144 / 384 blocks - and the LayerNorm launch that follows anyway finishes them (bias + slabs + residual, in place,
    // fixed order; layernorm_slab_kernel).  r02, encoder of 1 / 2 / 4 crops: 1.07 / 1.07 / 1.12 -> 0.88 / 0.90 / 1.01 ms
    // (one crop: FC2 28.3 -> 9.3 us, O-proj 11.8 -> 7.7, the LayerNorm behind them 6.6 -> 10.3)
    // The split then shrinks until its slabs fit the slab buffer (round_up(max_batch, 128) * 12288 floats), so the (O-proj,
    // FC2) splits depend on max_batch too.  max_batch <= 128: one crop (3, 8), two (3, 4), three (3, 2), four and five
    // (1, 2), six unsplit; max_batch 129 .. 256: one and two crops (3, 8), three to five (3, 4), six (3, 2).
    static const int enc_split_env = env_int("MOCR_ENC_SPLITK", 1);
    const long long blocks64 = (long long)((M + 63) / 64) * (D / 64);
    pl.split_o = 1; pl.split_2 = 1;
    static const int enc_split_blocks = env_int("MOCR_ENC_SPLITK_BLOCKS", 0);      // largest unsplit 64 x 64 grid that is split (0: one block per CU)
    if (enc_split_env && !enc_tile_env && !e->calib && pl.to == 64 && blocks64 <= (enc_split_blocks ? enc_split_blocks : e->num_cus)) {
        pl.split_o = 3; pl.split_2 = 8;
        while (pl.split_2 > 1 && (long long)M * D * pl.split_2 > e->slab_cap) pl.split_2 >>= 1;
        if ((long long)M * D * pl.split_o > e->slab_cap) pl.split_o = 1;
        if (pl.split_2 < 2) pl.split_2 = 1;
    }
    // bf16, all four layer GEMMs on the persistent kernel: the 24 LayerNorms between them are FOLDED into those GEMMs
    // (kernels_gemm_pers.h LNF; r03: 25 launches of 38-40 us were 7.5 % of the encoder at batch 256).  Xn then holds x itself
    // as bf16; only the final LayerNorm (the encoder's output) is a launch.
    pl.fold = false;
    if constexpr (sizeof(T) == 2) {
        static const int fold_env = env_int("MOCR_ENC_LN_FOLD", 1);
        auto folds = [](int code) { const TileCode* t = tile_code(code); return t && t->product_persistent(); };
        pl.fold = fold_env && !(e->cfg.flags & MOCR_FLAG_NO_LN_FOLD) && folds(pl.tq) && folds(pl.to) && folds(pl.t1) && folds(pl.t2) &&
                  D == 768 && e->w.enc[0].wqkv_f && !e->calib && (e->fold_ok || (e->cfg.flags & MOCR_FLAG_FORCE_LN_FOLD));
    }
    return pl;
}

// The encoder's front end: gray [n, IMG, IMG] -> patches T [n * 196, 256] (patchify) -> x f32 [n * 197, 768] (CLS rows + patch
// embedding).  tile: the patch embedding's tile code, 0 = the plan's.  `patches` holds round_up(n * 196, 128) rows (the GEMM
// stages whole tiles of A).  run_encoder and mocr_op_embed both come through here.
template <typename T>
void encoder_front(mocr_engine* e, const uint8_t* d_gray, int n, void* patches, float* x, int tile) {
    const int D = e->D, S = e->S, P = e->cfg.patch_size, IMG = e->cfg.image_size, NP = e->G * e->G;
    auto& w = e->w;
    {
        const long long total = (long long)n * IMG * e->G;
        ProfScope ps(e, "patchify", 0, (double)n * IMG * IMG * (1 + sizeof(T)));
        hipLaunchKernelGGL((patchify_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, d_gray,
                           w.lut, reinterpret_cast<T*>(patches), n, IMG, P);
        HIPCHECK(hipGetLastError());
    }
    {
        ProfScope ps(e, "cls_rows", 0, (double)n * D * 4);
        hipLaunchKernelGGL(cls_rows_kernel, dim3((n * D + 255) / 256), dim3(256), 0, e->stream, w.cls, w.pos_enc, x, n, S, D);
        HIPCHECK(hipGetLastError());
    }
    GemmCall embed = gemm_call("gemm_patch_embed", patches, P * P, w.wpe, w.bpe, x, D, n * NP, D, P * P, EPI_PATCH,
                               tile ? tile : encoder_plan<T>(e, n).embed_tile);
    embed.pos = w.pos_enc; embed.patches = NP;
    gemm<T>(e, embed);
}

// x += bias + the nslab fp32 slabs (slab_stride floats apart), in place, then out = LayerNorm(x): what finishes a layer GEMM
// split over K (layernorm_slab_kernel)
template <typename T>
void layernorm_slab(mocr_engine* e, float* x, const float* slabs, int nslab, long long slab_stride, const float* bias, const float* g,
                    const float* b, void* out, int M) {
    ProfScope ps(e, "layernorm_slab", 0, (double)M * e->D * (4.0 * (nslab + 2) + sizeof(T)));
    hipLaunchKernelGGL((layernorm_slab_kernel<T, 768>), dim3((M + 3) / 4), dim3(256), 0, e->stream, x, slabs, nslab, slab_stride, bias,
                       g, b, reinterpret_cast<T*>(out), M, e->cfg.ln_eps);
    HIPCHECK(hipGetLastError());
}

// (enc_out: where the final LayerNorm writes the n encodings; null = ENC)
template <typename T>
void run_encoder(mocr_engine* e, const uint8_t* d_gray, int n, void* enc_out = nullptr) {
    const int D = e->D, F = e->F, S = e->S, M = n * S;
    auto& w = e->w;
    const EncPlan pl = encoder_plan<T>(e, n);
    const int ETQ = pl.tq, ETO = pl.to, ET1 = pl.t1, ET2 = pl.t2, split_o = pl.split_o, split_2 = pl.split_2;
    const bool fold = pl.fold;
    const int gq = pl.gq, g1 = pl.g1;      // column groups of QKV's / FC1's tile order
    encoder_front<T>(e, d_gray, n, e->Hb, e->X, pl.embed_tile);
    const float* pend_bias = nullptr;      // bias of a split GEMM whose slabs the next LayerNorm has to add to X
    int pend_slabs = 0;
    auto norm = [&](const float* g, const float* b, void* out) {
        if (e->calib && !pend_slabs) calib_observe(e, M);
        if (!pend_slabs) { layernorm<T>(e, e->X, g, b, out, M); return; }
        layernorm_slab<T>(e, e->X, e->slabs, pend_slabs, (long long)M * D, pend_bias, g, b, out, M);
        pend_slabs = 0;
    };
    if (fold) {
        ProfScope ps(e, "ln_prep", 0, (double)M * D * 6);
        hipLaunchKernelGGL((ln_prep_kernel<768>), dim3((M + 3) / 4), dim3(256), 0, e->stream, e->X, reinterpret_cast<bf16_t*>(e->Xn),
                           e->ln_part, M);
        HIPCHECK(hipGetLastError());
    }
    // a layer GEMM split over K: fp32 slabs on the 64 x 64 kernel, the bias left to the LayerNorm launch behind it
    auto into_slabs = [&](GemmCall c, int split) {
        pend_bias = c.bias; pend_slabs = split;
        c.bias = nullptr; c.resid = nullptr; c.out = e->slabs; c.epi = EPI_SLAB; c.tile = 64; c.split = split; c.slab_stride = (long long)M * D;
        return c;
    };
    for (int l = 0; l < e->cfg.enc_layers; ++l) {
        const EncLayerW& L = w.enc[l];
        GemmCall qkv = gemm_call("gemm_enc_qkv", e->Xn, D, L.wqkv, L.bqkv, e->QKV, 3 * D, M, 3 * D, D, EPI_BIAS, ETQ);
        GemmCall oproj = gemm_call("gemm_enc_oproj", e->CTX, D, L.wo, L.bo, e->X, D, M, D, D, EPI_BIAS_RESID, ETO);
        GemmCall fc1 = gemm_call("gemm_enc_fc1", e->Xn, D, L.w1, L.b1, e->Hb, F, M, F, D, EPI_BIAS_GELU, ET1);
        GemmCall fc2 = gemm_call("gemm_enc_fc2", e->Hb, F, L.w2, L.b2, e->X, D, M, D, F, EPI_BIAS_RESID, ET2);
        qkv.group_n = gq; fc1.group_n = g1; oproj.resid = e->X; fc2.resid = e->X;
        // folded: QKV / FC1 read the rows' statistics and take the folded weights, O-proj / FC2 emit x as bf16 and its statistics
        const LnFold use_q{e->ln_part, L.sqkv, nullptr}, use_1{e->ln_part, L.s1, nullptr}, emit{e->ln_part, nullptr, e->Xn};
        if (fold) {
            qkv.W = L.wqkv_f; qkv.bias = L.bqkv_f; qkv.lnf = &use_q;
            fc1.W = L.w1_f; fc1.bias = L.b1_f; fc1.lnf = &use_1;
            oproj.lnf = &emit; fc2.lnf = &emit;
        }
        if (!fold) norm(L.ln1g, L.ln1b, e->Xn);
        gemm<T>(e, qkv);
        enc_attention<T>(e, e->QKV, e->CTX, n, pl.impl, pl.ysplit);
        gemm<T>(e, split_o > 1 ? into_slabs(oproj, split_o) : oproj);
        if (!fold) norm(L.ln2g, L.ln2b, e->Xn);
        gemm<T>(e, fc1);
        gemm<T>(e, split_2 > 1 ? into_slabs(fc2, split_2) : fc2);
    }
    norm(w.lnfg, w.lnfb, enc_out ? enc_out : e->ENC);
}

// ---------------------------------------------------------------------------------------- decoder
static int dec_tile(int rows) {
    static const int forced = env_int("MOCR_DEC_TILE", 0);
    // 128 x 128 tiles from 1024 rows (r02: from 512 - at 256 rows the 64 x 64 tiles need a third of the split-K slabs, 113 -> 101
    // ms for an isolated 256-crop batch.  r04, tools/r04_dectile_ab.sh, isolated batches, 64 / 128 tiles: 512 rows 128.0 / 134.3
    // ms, 640 rows 143.4 / 147.4, 768 rows 157.5 / 162.7, 1024 rows 199.8 / 195.4, 1280 rows 229 / 224)
    // (mocr_decode_plan: "regime tile" = this rule on the batch's regime, "launch tile" = on the rows of the launch)
    static const int fat = env_int("MOCR_DEC_FAT_ROWS", 1024);
    if (forced) return forced;
    return rows >= fat ? 128 : 64;
}

// The tile a decode-step GEMM is LAUNCHED on: the tile size does not touch a sum (same K-tiles, same order; the split over K
// stays the regime's, pick_split), so a compacted batch takes the tile of the rows it has left (MOCR_NEUTRAL_BY_ROWS >= 2, the
// default; r04, tools/r04_neutral_ab.sh, mixed-lengths leg, by regime / ring depth + query blocks by rows / + tile by rows:
// 11.96 / 12.12 / 12.39 k crops/s, ids bit-identical to the uncompacted engine in all three).
static int dec_launch_tile(const mocr_engine* e, int rows) {
    static const int neutral_by_rows = env_int("MOCR_NEUTRAL_BY_ROWS", 2);
    return dec_tile(neutral_by_rows >= 2 ? rows : e->rrows(rows));
}

static int pick_split(int N, int K, int kt, int rows, long long slab_cap_per_row) {
    // Split K until ~`target` blocks cover the chip, bounded by the K-tiles and by the slab buffer.
    // Every extra slab is an fp32 [rows,N] write plus a read by the consumer, so fat batches
    // (many row tiles) split less.
    // measured (r01): 150 for 64..1024 rows; fat batches (>= 2048 rows) gain from one more halving of K
    // (FC2 at 4096 rows: 48 -> 33 us: 192 tiles -> 384 blocks).  r02: 200 instead of 300 there - the same split at 4096
    // rows, but the N = 768 projections of a 2560-row batch (120 tiles) stop at 2 slabs instead of 4: the add + LayerNorm
    // behind them is bound by its slab traffic (bench 6.30-6.36 k -> 6.44-6.45 k crops/s; targets 60 / 100 / 450 / 600: 6.30 /
    // 6.32 / 6.35 / 6.10 k)
    static const int target_env = env_int("MOCR_DEC_BLOCKS", 0);
    // (r04, with the four-slot rings of lone batches, tools/r04_decblocks_small_ab.sh, targets 150 / 100: 96 rows 58.4 / 56.4 ms,
    // 128 rows 66.3 / 63.0, 40 / 64 / 192 / 256 rows equal; 320 and 768 rows lose with 100)
    // (mocr_decode_plan: the five "K slices".  Over the graph grid the N = 768 GEMMs reach two slabs at 1792 rows - 84 tiles x 2
    // >= 150 -, return to four at 2048 - 96 x 2 < 200 - and stay at two from 2304)
    const int target = target_env ? target_env : (rows >= 2048 ? 200 : rows <= 128 ? 100 : 150);
    const int tile = dec_tile(rows);
    const int tiles = (N / tile) * ((rows + tile - 1) / tile);
    const int ktiles = K / kt;
    int split = 1;
    while (tiles * split < target && split * 2 <= ktiles && ktiles % (split * 2) == 0 && (long long)(split * 2) * N <= slab_cap_per_row)
        split *= 2;
    if (tiles * split * 3 <= target * 2 && ktiles % (split * 3) == 0 && (long long)(split * 3) * N <= slab_cap_per_row) split *= 3;
    return split;
}

// K slices of a decode-step GEMM [rows, N] = A [rows, K] W^T: by the batch's regime, so that a compacted batch keeps its sums
// (the slab buffer holds 12288 floats per row whatever max_batch is, so the split does not depend on the engine's size)
template <typename T>
static int dec_split(const mocr_engine* e, int N, int K, int rows) {
    return pick_split(N, K, 128 / (int)sizeof(T), e->rrows(rows), e->slab_cap / e->Bp);
}
// FC1 unsplit: bias + GELU in the GEMM's epilogue (EPI_BIAS_GELU) instead of one slab and a bias_gelu launch
template <typename T>
static bool dec_fc1_fused(const mocr_engine* e, int rows) { return dec_split<T>(e, e->F, e->D, rows) == 1; }
// The LM head unsplit on a 64 / 128 tile: its epilogue reduces every N-tile to candidates (EPI_ARGMAX and its scored / masked
// forms) - unless the caller wants the logits or the batch is a beam batch, which decode_step checks itself
template <typename T>
static bool dec_head_fused(const mocr_engine* e, int rows) {
    return !(e->cfg.flags & MOCR_FLAG_NO_FUSED_ARGMAX) && tile_is(dec_launch_tile(e, rows), GemmKind::Tile) && dec_split<T>(e, e->V, e->D, rows) == 1;
}

template <typename T>
int dec_gemm(mocr_engine* e, const char* name, const void* A, int lda, const void* W, int N, int K, int rows) {
    const int split = dec_split<T>(e, N, K, rows);
    GemmCall c = gemm_call(name, A, lda, W, nullptr, e->slabs, N, rows, N, K, EPI_SLAB, dec_launch_tile(e, rows));
    c.split = split; c.slab_stride = (long long)e->Bp * N;
    gemm<T>(e, c);
    return split;
}

// The row-wise launches of the decode step are split in two: building the argument block from the engine's buffers, and
// launching from an argument block.  The decode step does both; the operator test hooks (mocr_op_dec_*) fill the block
// with their own device buffers and go through the same launch.
struct DecAddLnArgs {
    const float* slabs; int nslab; long long slab_stride;
    const float* bias; const float* resid; const float* g; const float* b;
    float* out_f32; void* out_t; int rows; bool gelu;
    void* cache; uint8_t* cache8; float inv8; long long cstride;      // latent cache row (T or e4m3) at rowmap[slot], step[slot]
    const int* step; const int* rowmap;
};

template <typename T>
void launch_dec_add_ln(mocr_engine* e, const DecAddLnArgs& a) {
    ProfScope ps(e, "dec_add_ln", 0, (double)a.rows * e->D * 4 * (a.nslab + 3));
    if (a.gelu)
        hipLaunchKernelGGL((dec_add_ln_kernel<T, 768, true>), dim3(a.rows), dim3(192), 0, e->stream, a.slabs, a.nslab,
                           a.slab_stride, a.bias, a.resid, a.g, a.b, a.out_f32, reinterpret_cast<T*>(a.out_t), a.rows, e->cfg.ln_eps,
                           reinterpret_cast<T*>(a.cache), a.cstride, a.step, a.cache8, a.inv8, a.rowmap);
    else
        hipLaunchKernelGGL((dec_add_ln_kernel<T, 768, false>), dim3(a.rows), dim3(192), 0, e->stream, a.slabs, a.nslab,
                           a.slab_stride, a.bias, a.resid, a.g, a.b, a.out_f32, reinterpret_cast<T*>(a.out_t), a.rows, e->cfg.ln_eps,
                           reinterpret_cast<T*>(a.cache), a.cstride, a.step, a.cache8, a.inv8, a.rowmap);
    HIPCHECK(hipGetLastError());
}

template <typename T>
void dec_add_ln(mocr_engine* e, int nslab, int N, const float* bias, const float* resid, const float* g, const float* b,
                float* out_f32, void* out_t, int rows, bool gelu, int cache_layer = -1, void* hist = nullptr, int hist_len = 0) {
    DecAddLnArgs a{};
    a.slabs = e->slabs; a.nslab = nslab; a.slab_stride = (long long)e->Bp * N;
    a.bias = bias; a.resid = resid; a.g = g; a.b = b; a.out_f32 = out_f32; a.out_t = out_t; a.rows = rows; a.gelu = gelu;
    a.cstride = (long long)e->cfg.max_len * e->D;
    a.step = e->step; a.rowmap = e->rowmap;
    if (cache_layer >= 0) {
        if (e->fp8attn) {
            a.cache8 = e->x8cache + (size_t)cache_layer * e->Bp * a.cstride;
            a.inv8 = 1.0f / e->w.sx_self[cache_layer];
        } else {
            a.cache = reinterpret_cast<T*>(e->xcache) + (size_t)cache_layer * e->Bp * a.cstride;
        }
    }
    if (hist) {                     // token positions: the row as T at hist[rowmap[slot]][step[slot]], rows of hist_len positions
        a.cache = hist; a.cstride = (long long)hist_len * e->D;      // (never together with a cache layer)
    }
    launch_dec_add_ln<T>(e, a);
}

// out T = gelu(sum of the FC1 slabs + bias): FC1 when it is split over K
template <typename T>
void launch_dec_bias_gelu(mocr_engine* e, const float* slabs, int nslab, long long slab_stride, const float* bias, void* out,
                          int rows, int N) {
    ProfScope ps(e, "dec_bias_gelu", 0, (double)rows * N * (4.0 * nslab + sizeof(T)));
    hipLaunchKernelGGL((dec_bias_gelu_kernel<T>), dim3((unsigned)(((long long)rows * N / 4 + 255) / 256)), dim3(256), 0, e->stream,
                       slabs, nslab, slab_stride, bias, reinterpret_cast<T*>(out), rows, N);
    HIPCHECK(hipGetLastError());
}

static DecState make_state(mocr_engine* e, int max_len, const int* forced, int forced_T, float* logits_out, int n_real,
                           const DecMode& m = DecMode{}) {
    DecState st{};
    st.n_real = n_real;
    st.ids = e->ids; st.step = e->step; st.finished = e->finished; st.len = e->len; st.n_unfinished = e->n_unf;
    st.forced = forced; st.forced_T = forced_T; st.logits_out = logits_out;
    st.ids_ld = e->cfg.max_len; st.max_len = max_len;
    st.start_id = e->cfg.start_id; st.eos_id = e->cfg.eos_id; st.pad_id = e->cfg.pad_id;
    st.rowmap = e->rowmap;
    st.scores = m.level >= 1 ? e->scores : nullptr;
    st.alt_ids = m.level >= 2 ? e->alt_ids : nullptr; st.alt_logp = m.level >= 2 ? e->alt_logp : nullptr;
    st.tok_mask = m.mask ? e->tok_table : nullptr; st.set_of_row = m.mask ? e->set_of_row : nullptr;
    if (m.ngram) {        // the masked kernels read the row's own mask; the sets become the base the NGRAM token kernel rebuilds it from
        st.tok_mask = e->row_mask; st.set_of_row = e->row_ident;
        st.row_mask = e->row_mask; st.base_mask = e->tok_table; st.base_set_of_row = e->set_of_row; st.ngram_of_row = e->ngram_of_row;
    }
    if (m.prefix) { st.prefix = e->prefix; st.prefix_len = e->prefix_len; st.prefix_ld = e->cfg.max_len; st.tgt_val = e->tgt_val; }
    return st;
}

// The token kernel's buffers; the embedding tables and their LayerNorm are always the engine's weights.
struct DecTokenArgs {
    const float* slabs; int nslab; long long slab_stride;
    const float* vbias;                                   // LM-head bias (slab path)
    const float* cand_val; const int* cand_idx; int ncand;   // per-tile candidates of the fused LM head (ncand > 0)
    const float* cand_sum;                                // scored steps (st.scores set) on the candidate path: the tiles' exp sums
    const float* top_val; const int* top_idx;             // alternatives steps (st.alt_ids set) on the candidate path: the tiles' four best
    float* x_f32; void* x_t;
    void* cache; uint8_t* cache8; float inv8; long long cstride;   // layer-0 latent cache row (T or e4m3), indexed by row
    DecPenAutomata aut;                                   // token automata (the six set: the AUTOMATON form; the state then has the per-row masks;
                                                          // edge_weight and default_next set too: the SOFT form; pen set: the PEN form,
                                                          // in which the eight may be null)
};

// dec_token_kernel (kernels_decode.h; T, 768, FIRST, SCORES, TOPK, MASK, NGRAM, AUTOMATON, SOFT, PEN): the start token's kernel (it
// has nothing to score or to mask), then level (ids, SCORES, SCORES + TOPK) x kind - plain, MASK, NGRAM, AUTOMATON, SOFT, PEN, each
// kind the one before plus its flag.  A row carries its profile name.
struct TokenArgs { bool first, scores, topk, mask, ngram, automaton, soft, pen; const char* name; };
constexpr bool operator==(const TokenArgs& a, const TokenArgs& b) {
    return a.first == b.first && a.scores == b.scores && a.topk == b.topk && a.mask == b.mask && a.ngram == b.ngram &&
           a.automaton == b.automaton && a.soft == b.soft && a.pen == b.pen;
}
// (the table's rows and the run-time key are both made here, so a key is always a row)
constexpr TokenArgs token_form(bool first, int level, int kind, const char* name = nullptr) {
    if (first) return TokenArgs{true, false, false, false, false, false, false, false, name};
    return TokenArgs{false, level >= 1, level >= 2, kind >= 1, kind >= 2, kind >= 3, kind >= 4, kind >= 5, name};
}
constexpr std::array<TokenArgs, 19> token_forms() {
    constexpr const char* names[3][6] = {
        {"dec_token", "dec_token_m", "dec_token_ng", "dec_token_am", "dec_token_sw", "dec_token_rp"},
        {"dec_token_lse", "dec_token_lse_m", "dec_token_lse_ng", "dec_token_lse_am", "dec_token_lse_sw", "dec_token_lse_rp"},
        {"dec_token_topk", "dec_token_topk_m", "dec_token_topk_ng", "dec_token_topk_am", "dec_token_topk_sw", "dec_token_topk_rp"}};
    std::array<TokenArgs, 19> a{};
    int n = 0;
    a[n++] = token_form(true, 0, 0, "dec_token_first");
    for (int level = 0; level < 3; ++level)
        for (int kind = 0; kind < 6; ++kind) a[n++] = token_form(false, level, kind, names[level][kind]);
    return a;
}
// The operator hooks come with a bare DecState, so the form is read off the pointers: scores / alternatives, and the richest of
// token sets / per-row masks / automaton tables / weights / seen words that is set (make_state and dec_token set them from the
// batch's DecMode).
static TokenArgs token_key(bool first, const DecState& st, const DecTokenArgs& a) {
    return token_form(first, st.alt_ids ? 2 : st.scores ? 1 : 0,
                      a.aut.pen.seen_mask ? 5 : a.aut.edge_weight ? 4 : a.aut.state ? 3 : st.row_mask ? 2 : st.tok_mask ? 1 : 0);
}
template <typename T> struct TokenFamily {
    using Args = TokenArgs;
    struct Launch {
        mocr_engine* e; const DecState& st; const DecTokenArgs& a; int n;
        template <typename K> void operator()(K kernel) const {
            auto& w = e->w;
            const bool cand = a.ncand > 0, scored = cand && (st.scores || st.alt_ids), alts = cand && st.alt_ids;
            hipLaunchKernelGGL(kernel, dim3(n), dim3(256), 0, e->stream, a.slabs, a.nslab, a.slab_stride, a.vbias, e->V, st, w.word, w.type0,
                               w.posd, w.embg, w.embb, a.x_f32, reinterpret_cast<T*>(a.x_t), e->cfg.ln_eps, reinterpret_cast<T*>(a.cache),
                               a.cstride, cand ? a.cand_val : nullptr, cand ? a.cand_idx : nullptr, a.ncand, a.cache8, a.inv8,
                               scored ? a.cand_sum : nullptr, alts ? a.top_val : nullptr, alts ? a.top_idx : nullptr, a.aut);
        }
    };
    using Kernel = Sliced<Launch>;
    static constexpr std::array<Args, 19> forms = token_forms();
    static_assert(forms[18].topk && forms[18].pen, "token_forms fills its table");
    template <size_t I> static constexpr auto kernel() {
        constexpr Args f = forms[I];
        return dec_token_kernel<T, 768, f.first, f.scores, f.topk, f.mask, f.ngram, f.automaton, f.soft, f.pen>;
    }
    static constexpr int lds(const Args&) { return 0; }
};

template <typename T, bool FIRST>
void launch_dec_token(mocr_engine* e, const DecState& st, const DecTokenArgs& a, int n) {
    const TokenArgs key = token_key(FIRST, st, a);
    ProfScope ps(e, find_row<TokenFamily<T>>(key)->name, 0, FIRST ? 0.0 : (double)n * e->V * 4 * a.nslab);
    find_form<TokenFamily<T>>(key).kernel({e, st, a, n});
    HIPCHECK(hipGetLastError());
}

// The step's token-kernel (or selection) arguments on the engine's buffers: the LM head's slabs, the embedding of the chosen
// token and its layer-0 latent cache row
static DecTokenArgs dec_token_args(mocr_engine* e, int nslab, int n) {
    const bool lat = e->use_latent(e->rrows(n));
    DecTokenArgs a{};
    a.slabs = e->slabs; a.nslab = nslab; a.slab_stride = (long long)e->Bp * e->V; a.vbias = e->w.bv;
    a.x_f32 = e->x_f32; a.x_t = e->x_t;
    a.cache = (lat && !e->fp8attn) ? e->xcache : nullptr;
    a.cache8 = (lat && e->fp8attn) ? e->x8cache : nullptr;
    a.inv8 = (lat && e->fp8attn) ? 1.0f / e->w.sx_self[0] : 0.f;
    a.cstride = (long long)e->cfg.max_len * e->D;
    return a;
}

// The token kernel of a batch in mode `m` (the start token's, FIRST, is the same for every mode)
template <typename T, bool FIRST>
void dec_token(mocr_engine* e, const DecState& st, const DecMode& m, int nslab, int n, int ncand = 0) {
    DecTokenArgs a = dec_token_args(e, nslab, n);
    a.cand_val = e->cand_val; a.cand_idx = e->cand_idx; a.ncand = ncand; a.cand_sum = e->cand_sum;
    a.top_val = e->top_val; a.top_idx = e->top_idx;
    if (!FIRST && m.automaton) {
        static_cast<DecAutomata&>(a.aut) = DecAutomata{e->aut_edge_begin, e->aut_edge_token, e->aut_edge_next, e->aut_accepting, e->aut_base_of_row, e->aut_state};
        if (m.soft) { a.aut.edge_weight = e->aut_edge_weight; a.aut.default_next = e->aut_default_next; }
        if (m.penalty) a.aut.pen = DecPenalty{e->seen_mask, e->penalty_of_row};
    }
    launch_dec_token<T, FIRST>(e, st, a, n);
}

// ---- beam search: the selection and the cache reorder that end a beam step (kernels_beam.h) ----
static BeamState make_beam_state(mocr_engine* e, const mocr_beam_config& c, bool tokens, bool trails) {
    BeamState bs{};
    if (tokens) { bs.beam_logp = e->beam_logp; bs.hyp_logp = e->hyp_logp; bs.tok_mask = e->tok_table; bs.set_of_row = e->set_of_row; }
    if (trails) { bs.beam_trail = e->beam_trail; bs.hyp_trail = e->hyp_trail; }
    bs.beam_score = e->beam_score; bs.parent = e->beam_parent;
    bs.hyp_ids = e->hyp_ids; bs.hyp_len = e->hyp_len; bs.hyp_score = e->hyp_score; bs.heuristic_open = e->heuristic_open;
    bs.length_penalty = c.length_penalty; bs.early_stopping = c.early_stopping; bs.ngram = c.no_repeat_ngram_size;
    return bs;
}

// the trailing argument of the automaton form, on the engine's tables and the bound lane's states
// (`soft`: a crop of the batch brings a soft handle - the arena's soft part too, and with it the selection's SOFT form)
static BeamSoftAutomata make_beam_automata(mocr_engine* e, bool soft) {
    BeamSoftAutomata a{};
    static_cast<BeamAutomata&>(a) =
        BeamAutomata{e->aut_edge_begin, e->aut_edge_token, e->aut_edge_next, e->aut_accepting, e->aut_base_of_row, e->aut_state, e->hyp_state};
    if (soft) { a.edge_weight = e->aut_edge_weight; a.default_next = e->aut_default_next; }
    return a;
}

// beam_select_kernel (kernels_beam.h; T, K, TOK, TRAIL, AUT, SOFT): K = 2 .. 4 x kind - plain, TOK, AUT (a token form), SOFT, each
// kind the one before plus its flag - without and with the two trails.  A row carries its profile name.
struct BeamArgs { int K; bool tok, trail, aut, soft; const char* name; };
constexpr bool operator==(const BeamArgs& a, const BeamArgs& b) {
    return a.K == b.K && a.tok == b.tok && a.trail == b.trail && a.aut == b.aut && a.soft == b.soft;
}
constexpr std::array<BeamArgs, 24> beam_forms() {
    constexpr const char* names[4][2] = {{"beam_select", "beam_select"}, {"beam_select_tok", "beam_select_tok"},
                                         {"beam_select_am", "beam_select_am_tr"}, {"beam_select_sw", "beam_select_sw_tr"}};
    std::array<BeamArgs, 24> a{};
    int n = 0;
    for (int K = 2; K <= 4; ++K)
        for (int kind = 0; kind < 4; ++kind)
            for (int trail = 0; trail < 2; ++trail) a[n++] = BeamArgs{K, kind >= 1, trail != 0, kind >= 2, kind >= 3, names[kind][trail]};
    return a;
}
template <typename T> struct BeamSelectFamily {
    using Args = BeamArgs;
    struct Launch {
        mocr_engine* e; const DecState& st; const BeamState& bs; const DecTokenArgs& a; int n, K; const BeamSoftAutomata& aut;
        template <typename Kn> void operator()(Kn kernel) const {
            auto& w = e->w;
            hipLaunchKernelGGL(kernel, dim3((n + K - 1) / K), dim3(256), 0, e->stream, a.slabs, a.nslab, a.slab_stride, a.vbias, e->V, st, bs, n,
                               w.word, w.type0, w.posd, w.embg, w.embb, a.x_f32, reinterpret_cast<T*>(a.x_t), e->cfg.ln_eps,
                               reinterpret_cast<T*>(a.cache), a.cstride, a.cache8, a.inv8, aut);
        }
    };
    using Kernel = Sliced<Launch>;
    static constexpr std::array<Args, 24> forms = beam_forms();
    static_assert(forms[23].K == 4 && forms[23].soft && forms[23].trail, "beam_forms fills its table");
    template <size_t I> static constexpr auto kernel() { constexpr Args f = forms[I]; return beam_select_kernel<T, f.K, f.tok, f.trail, f.aut, f.soft>; }
    static constexpr int lds(const Args&) { return 0; }
};

// n decode slots = groups of K (a trailing partial group is padding); the LM head's slabs, by slot, are in `a`
template <typename T>
void launch_beam_select(mocr_engine* e, const DecState& st, const BeamState& bs, const DecTokenArgs& a, int n, int K,
                        const BeamSoftAutomata& aut = BeamSoftAutomata{}) {
    if (e->D != 768 || e->V != 6144 || st.ids_ld > BEAM_HIST || st.max_len > st.ids_ld || a.nslab < 1)
        throw ArgError{"beam search needs hidden 768, vocab 6144 and max_len <= 320", MOCR_ERR_UNSUPPORTED};
    // the token form when the state carries any of its four arrays (make_beam_state sets them from the batch's DecMode)
    const bool tok = bs.beam_logp || bs.hyp_logp || bs.tok_mask || bs.set_of_row;
    if ((bs.beam_logp == nullptr) != (bs.hyp_logp == nullptr) || (bs.tok_mask == nullptr) != (bs.set_of_row == nullptr))
        throw ArgError{"beam_select: the two token histories, and the set table with the rows' sets, come in pairs", MOCR_ERR_ARG};
    // ... and the trail form when it carries the two trails (a batch that records token positions)
    const bool trail = bs.beam_trail || bs.hyp_trail;
    if ((bs.beam_trail == nullptr) != (bs.hyp_trail == nullptr))
        throw ArgError{"beam_select: the two trails come as a pair", MOCR_ERR_ARG};
    // ... and the automaton form, a token form, when the trailing argument is set (all seven pointers or none)
    if (aut.state) {
        if (!aut.edge_begin || !aut.edge_token || !aut.edge_next || !aut.accepting || !aut.base_of_row || !aut.hyp_state)
            throw ArgError{"beam_select: the automaton tables, the rows' bases and the two state arrays come together", MOCR_ERR_ARG};
        if ((aut.edge_weight == nullptr) != (aut.default_next == nullptr))
            throw ArgError{"beam_select: edge_weight and default_next come as a pair", MOCR_ERR_ARG};
    }
    // ... and its SOFT form with the weights: inside the beams' scores, open states
    const BeamArgs key{K, tok || aut.state, trail, aut.state != nullptr, aut.state && aut.edge_weight, nullptr};
    const BeamArgs* const row = find_row<BeamSelectFamily<T>>(key);
    if (!row) throw ArgError{"num_beams must be 2 .. 4", MOCR_ERR_ARG};
    ProfScope ps(e, row->name, 0, (double)n * e->V * 4 * a.nslab);
    find_form<BeamSelectFamily<T>>(key).kernel({e, st, bs, a, n, K, aut});
    HIPCHECK(hipGetLastError());
}

// max_pos bounds every slot's step (positions 0 .. step - 1 move): it sizes the grid
static void launch_beam_permute(mocr_engine* e, const BeamPermuteView& v, int layers, int K, const int* parent, const int* rowmap,
                                const int* finished, const int* step, int n, int max_pos) {
    if (v.pos_bytes < 16 || v.pos_bytes % 16 || layers < 1 || v.segs < 1 || max_pos < 1)
        throw ArgError{"beam_permute: positions of whole 16-byte pieces", MOCR_ERR_ARG};
    const int groups = n / K;
    if (groups < 1) return;
    const long long pieces = (long long)max_pos * v.pos_bytes / 16;
    const dim3 grid((unsigned)groups, (unsigned)(layers * v.segs), (unsigned)((pieces + 255) / 256));
    ProfScope ps(e, "beam_permute", 0, 2.0 * n * layers * v.segs * (double)max_pos * v.pos_bytes);
    switch (K) {
        case 2: hipLaunchKernelGGL(beam_permute_kernel<2>, grid, dim3(256), 0, e->stream, v, parent, rowmap, finished, step, n, max_pos); break;
        case 3: hipLaunchKernelGGL(beam_permute_kernel<3>, grid, dim3(256), 0, e->stream, v, parent, rowmap, finished, step, n, max_pos); break;
        case 4: hipLaunchKernelGGL(beam_permute_kernel<4>, grid, dim3(256), 0, e->stream, v, parent, rowmap, finished, step, n, max_pos); break;
        default: throw ArgError{"num_beams must be 2 .. 4", MOCR_ERR_ARG};
    }
    HIPCHECK(hipGetLastError());
}

// The end of a beam step on the engine's buffers: the selection over the LM head's slabs, then the reorder of whichever
// self-attention cache the batch's regime keeps (latent rows, their e4m3 form, or the classic K and V).
template <typename T>
void beam_finish_step(mocr_engine* e, const DecState& st, const DecMode& m, int nslab, int n, int t) {
    const int K = m.beam_cfg.num_beams;
    const bool lat = e->use_latent(e->rrows(n));
    const DecTokenArgs a = dec_token_args(e, nslab, n);
    launch_beam_select<T>(e, st, make_beam_state(e, m.beam_cfg, m.beam_tokens, m.positions), a, n, K,
                          m.beam_automaton ? make_beam_automata(e, m.soft) : BeamSoftAutomata{});
    // `t` bounds the step index of this launch from above only when it is exact (eager steps).  A captured graph passes
    // t = t_hi - 1 for every step of its bucket (decode_graph), and the bucket's last device step is t_hi itself
    // (t0 + steps <= 32 * bucket): behind it `step` is t_hi + 1 = t + 2 positions.  The grid is sized for that; the kernel
    // moves `step` positions, never more than the grid covers, and a live crop's step is below max_len.
    const int layers = e->cfg.dec_layers, max_pos = std::min(t + 2, st.max_len - 1);
    const long long ML = e->cfg.max_len;
    if (lat) {
        const long long pb = e->fp8attn ? e->D : (long long)e->D * sizeof(T);
        BeamPermuteView v{reinterpret_cast<char*>(e->fp8attn ? (void*)e->x8cache : e->xcache), (long long)e->Bp * ML * pb, ML * pb, 0, 1, (int)pb};
        launch_beam_permute(e, v, layers, K, e->beam_parent, e->rowmap, e->finished, e->step, n, max_pos);
    } else {
        const long long pb = 64 * (long long)sizeof(T);
        for (void* base : {e->kcache, e->vcache}) {
            BeamPermuteView v{reinterpret_cast<char*>(base), (long long)e->Bc * e->H * ML * pb, (long long)e->H * ML * pb, ML * pb, e->H, (int)pb};
            launch_beam_permute(e, v, layers, K, e->beam_parent, e->rowmap, e->finished, e->step, n, max_pos);
        }
    }
}

// non-temporal K/V loads from about 128 rows of the batch's regime (see dec_attn_params; mocr_decode_plan: field 22)
static bool dec_attn_nt(const mocr_engine* e, int n) {
    static const int nt_rows = env_int("MOCR_ATTN_NT_ROWS", 128);
    return e->rrows(n) >= nt_rows;
}

// The launch of the classic decode attention: NG (8-key groups a wave may own) is chosen here, from approx_len.
template <typename T, bool SELF>
void launch_dec_attn(mocr_engine* e, const DecAttnParams& p, int n, int approx_len) {
    const int H = e->H;
    ProfScope ps(e, SELF ? "dec_attn_self" : "dec_attn_cross", 4.0 * n * H * approx_len * 64,
                 2.0 * n * H * approx_len * 64 * sizeof(T));
    if (SELF) {
        // NG = 8-key groups a wave may own: pick the smallest variant that covers approx_len keys
        // (approx_len is an upper bound of every row's context length during this launch)
        const int need = ((approx_len + 3) / 4 + 7) / 8;
        if (need <= 3) hipLaunchKernelGGL((dec_attn_kernel<T, true, 3>), dim3(n * H), dim3(256), 0, e->stream, p);
        else if (need <= 5) hipLaunchKernelGGL((dec_attn_kernel<T, true, 5>), dim3(n * H), dim3(256), 0, e->stream, p);
        else if (need <= 8) hipLaunchKernelGGL((dec_attn_kernel<T, true, 8>), dim3(n * H), dim3(256), 0, e->stream, p);
        else if (need <= 10) hipLaunchKernelGGL((dec_attn_kernel<T, true, 10>), dim3(n * H), dim3(256), 0, e->stream, p);
        else throw ArgError{"max_len > 320 needs a larger NG", MOCR_ERR_UNSUPPORTED};
    } else {
        hipLaunchKernelGGL((dec_attn_kernel<T, false, 7>), dim3(n * H), dim3(256), 0, e->stream, p);
    }
    HIPCHECK(hipGetLastError());
}

// The parameter block of one decode attention launch.  slabs: [nslab][slab_rows][ldq] fp32; SELF: kc / vc = the layer's
// K / V cache [rows][H][max_len][64]; cross: kc = the cross K/V block [rows][S][NCKV] (layer = which column pair).
template <typename T, bool SELF>
DecAttnParams dec_attn_block(const mocr_engine* e, const float* slabs, long long slab_rows, int nslab, const float* bias,
                             const void* kc, const void* vc, int layer, const int* step, const int* rowmap, void* ctx, int n) {
    const int D = e->D, H = e->H;
    DecAttnParams p{};
    p.slabs = slabs; p.nslab = nslab;
    p.ldq = SELF ? 3 * D : D;
    p.slab_stride = slab_rows * p.ldq;
    p.bias = bias;
    if (SELF) {
        p.kbase = kc;
        p.vbase = vc;
        p.kv_batch_stride = (long long)H * e->cfg.max_len * 64;
        p.kv_head_stride = (long long)e->cfg.max_len * 64;
        p.kv_row_stride = 64;
        p.step = step;
    } else {
        p.kbase = reinterpret_cast<const char*>(kc) + (size_t)(layer * 2 * D) * sizeof(T);
        p.vbase = reinterpret_cast<const char*>(kc) + (size_t)(layer * 2 * D + D) * sizeof(T);
        p.kv_batch_stride = (long long)e->S * e->NCKV;
        p.kv_head_stride = 64;
        p.kv_row_stride = e->NCKV;
        p.cross_len = e->S;
    }
    p.ctx = ctx; p.H = H; p.scale = 0.125f;
    p.rowmap = rowmap;
    // K/V of a 64-row batch (2 layers x 197 keys x 3,072 B = 77 MB + the self cache) live in the Infinity Cache between
    // steps; from about 128 rows they no longer do and the non-temporal policy wins (r02, isolated batch: 256 rows
    // 100.2 -> 91.2 ms, 128 rows 69.1 -> 67.5 ms, 64 rows 49.8 -> 50.8 ms)
    p.nt = dec_attn_nt(e, n);
    return p;
}

template <typename T, bool SELF>
DecAttnParams dec_attn_params(mocr_engine* e, int layer, int nslab, int n, const float* bias) {
    const size_t per_layer = (size_t)e->Bc * e->H * e->cfg.max_len * 64;
    const void* kc = SELF ? reinterpret_cast<const char*>(e->kcache) + (size_t)layer * per_layer * sizeof(T) : e->CKV;
    const void* vc = SELF ? reinterpret_cast<const char*>(e->vcache) + (size_t)layer * per_layer * sizeof(T) : nullptr;
    return dec_attn_block<T, SELF>(e, e->slabs, e->Bp, nslab, bias, kc, vc, layer, e->step, e->rowmap, e->ctx_t, n);
}

template <typename T, bool SELF>
void dec_attn(mocr_engine* e, int layer, int nslab, int n, const float* bias, int approx_len) {
    launch_dec_attn<T, SELF>(e, dec_attn_params<T, SELF>(e, layer, nslab, n, bias), n, approx_len);
}

// The bf16 latent attention launch (r04).  Default: latent_attnT_kernel<.., 2> - 16-key tiles, the score tile transposed so that
// the softmax's probabilities feed P.X from registers (two barriers per tile; kernels_latent_t.h), THREE persistent blocks per
// CU on two-slot rings (52 KiB of LDS, 152 registers).  MOCR_FLAG_LATENT_TILE32 = r03's kernel shape, the A/B partner:
// latent_attn_kernel on 32-key tiles, one block per CU, three barriers per tile (kernels_latent.h).  Experiments build,
// MOCR_LAT_TK = 17: the default kernel on three-slot rings, two blocks per CU (-2 % in the bench); 16: latent_attn_kernel on
// 16-key tiles, two blocks per CU (the first half of r04; equal to 17 within noise).
struct LatentArgs { bool self; int v; };      // v: TK of latent_attn_kernel, NST of latent_attnT_kernel, unused (0) by the fp8 kernels
constexpr bool operator==(const LatentArgs& a, const LatentArgs& b) { return a.self == b.self && a.v == b.v; }
struct LatentFamily {          // latent_attn_kernel<SELF, TK>
    using Args = LatentArgs;
    using Kernel = void (*)(LatentParams);
    static constexpr Args forms[] = {{true, 32}, {false, 32}, LAB_ONLY({true, 16}, {false, 16})};
    template <size_t I> static constexpr Kernel kernel() { return latent_attn_kernel<forms[I].self, forms[I].v>; }
    static constexpr int lds(const Args& a) { return a.v == 32 ? LatCfg<32>::LDS : LatCfg<16>::LDS; }
};
struct LatentTFamily {         // latent_attnT_kernel<SELF, NST>
    using Args = LatentArgs;
    using Kernel = void (*)(LatentParams);
    static constexpr Args forms[] = {{true, 2}, {false, 2}, LAB_ONLY({true, 3}, {false, 3})};
    template <size_t I> static constexpr Kernel kernel() { return latent_attnT_kernel<forms[I].self, forms[I].v>; }
    static constexpr int lds(const Args& a) { return LATT_LDS_OF(a.v); }
};
struct Latent8Family {         // latent_attn_fp8_kernel<SELF>
    using Args = LatentArgs;
    using Kernel = void (*)(Latent8Params);
    static constexpr Args forms[] = {{true, 0}, {false, 0}};
    template <size_t I> static constexpr Kernel kernel() { return latent_attn_fp8_kernel<forms[I].self>; }
    static constexpr int lds(const Args&) { return LAT8_LDS; }
};
struct LatentT8Family {        // latent_attnT8_kernel<SELF>
    using Args = LatentArgs;
    using Kernel = void (*)(Latent8Params);
    static constexpr Args forms[] = {{true, 0}, {false, 0}};
    template <size_t I> static constexpr Kernel kernel() { return latent_attnT8_kernel<forms[I].self>; }
    static constexpr int lds(const Args&) { return LATT8_LDS; }
};

void launch_latent(mocr_engine* e, bool self, const LatentParams& p) {
    static const int lat_blocks = env_int("MOCR_LAT_BLOCKS", 0);      // persistent blocks (experiments; 0: one or two per CU by tile)
    const int per_cu = e->lat_tk == 32 ? 1 : e->lat_tk == 18 ? 3 : 2;
    const int grid = std::min(p.rows, lat_blocks > 0 ? lat_blocks : per_cu * e->num_cus);
    // lat_tk 18 (the default) / 17: latent_attnT_kernel on two / three ring slots; 16: latent_attn_kernel on 16-key tiles; anything
    // else, and whatever this build does not have: latent_attn_kernel on 32-key tiles
    auto f = find_form<LatentTFamily>({self, 20 - e->lat_tk});
    if (!f.kernel) f = find_form<LatentFamily>({self, e->lat_tk});
    if (!f.kernel) f = find_form<LatentFamily>({self, 32});
    hipLaunchKernelGGL(f.kernel, dim3(grid), dim3(256), f.lds, e->stream, p);
    HIPCHECK(hipGetLastError());
}

// The fp8 latent attention launch: latent_attnT8_kernel (r04: transposed score tile, one 32-key tile per iteration, two blocks per
// CU; kernels_latent_t8.h) or - MOCR_FLAG_LATENT_TILE32, the A/B partner - r02's latent_attn_fp8_kernel (two tiles per iteration
// on a five-slot ring, one block per CU).
void launch_latent8(mocr_engine* e, bool self, const Latent8Params& p) {
    static const int lat_blocks = env_int("MOCR_LAT_BLOCKS", 0);
    const bool tile32 = e->lat_tk == 32;
    const int grid = std::min(p.rows, lat_blocks > 0 ? lat_blocks : (tile32 ? 1 : 2) * e->num_cus);
    const auto f = tile32 ? find_form<Latent8Family>({self, 0}) : find_form<LatentT8Family>({self, 0});
    hipLaunchKernelGGL(f.kernel, dim3(grid), dim3(256), f.lds, e->stream, p);
    HIPCHECK(hipGetLastError());
}

// The latent attention block's buffers.  Like the decode helpers above it is built in one step - from the engine's state
// for one layer (latent_block_args), or from a caller's buffers (mocr_op_latent_block) - and launched from in another
// (launch_latent_block), so that the test hook runs the variants the decode step picks.
struct LatentBlockArgs {
    bool self; int n;
    int approx_len;                                  // the profiler's context length
    const void* xin; const void* wq; const float* bq; const void* wkT; const void* wv; const float* bv;
    const void* keys;                                // bf16 rows, or e4m3 bytes on an fp8 engine
    long long key_stride;                            // elements (bytes for e4m3) between two slots' first key
    int fixed_len;                                   // cross: keys per slot; self: step[0] + 1
    const int* step; const int* rowmap;
    float sx;                                        // fp8: key = e4m3 * sx
    void* q; void* qt; void* et; void* ctx;
};

// Latent attention of n rows: Qt [n,16,768] x keys (self: cached layer-input rows; cross: encoder
// output) -> Et [n,16,768].  bytes: the X rows streamed once (1,536 B per key).
void latent_attn(mocr_engine* e, const LatentBlockArgs& a) {
    const int n = a.n, approx_len = a.approx_len;
    if (e->fp8attn) {
        Latent8Params p{};
        p.qt = reinterpret_cast<const bf16_t*>(a.qt);
        p.out = reinterpret_cast<bf16_t*>(a.et);
        p.heads = e->H;
        p.rows = n;
        p.rowmap = a.rowmap;
        p.x8 = reinterpret_cast<const uint8_t*>(a.keys);
        p.x_batch_stride = a.key_stride;
        p.step = a.step;
        p.fixed_len = a.fixed_len;
        p.sx = a.sx;
        ProfScope ps(e, a.self ? "lat8_attn_self" : "lat8_attn_cross", 4.0 * n * 16 * approx_len * e->D,
                     (double)n * approx_len * e->D + 2.0 * n * e->H * e->D * 2);     // e4m3 keys + Qt in + Et out (12 heads, bf16)
        launch_latent8(e, a.self, p);
        return;
    }
    LatentParams p{};
    p.qt = reinterpret_cast<const bf16_t*>(a.qt);
    p.out = reinterpret_cast<bf16_t*>(a.et);
    p.heads = e->H;
    p.rows = n;
    p.rowmap = a.rowmap;
    p.x = reinterpret_cast<const bf16_t*>(a.keys);
    p.x_batch_stride = a.key_stride;
    p.step = a.step;
    p.fixed_len = a.fixed_len;
    ProfScope ps(e, a.self ? "lat_attn_self" : "lat_attn_cross", 4.0 * n * 16 * approx_len * e->D,
                 (double)n * approx_len * e->D * 2 + 2.0 * n * e->H * e->D * 2);     // keys + Qt in + Et out (12 heads)
    launch_latent(e, a.self, p);
}

// The fused query launch (kernels_qqt.h): blocks of 64 rows for batches of up to MOCR_QQT_BM64_ROWS rows (a 16-KiB K-tile, seven
// in flight, twice the blocks: r04, tools/r04_qqt_bm_ab.sh), of 128 rows above - there every CU has a block either way and the
// 128-row block reads each weight tile for twice the rows.  `regime_rows` = the row count the choice is made by.
struct QqtArgs { int bm; };
constexpr bool operator==(const QqtArgs& a, const QqtArgs& b) { return a.bm == b.bm; }
struct QqtFamily {             // dec_qqt_kernel<BM>
    using Args = QqtArgs;
    using Kernel = void (*)(QqtParams);
    static constexpr Args forms[] = {{64}, {128}};
    template <size_t I> static constexpr Kernel kernel() { return dec_qqt_kernel<forms[I].bm>; }
    static constexpr int lds(const Args&) { return 160 * 1024; }      // the limit: a launch asks for QqtCfg<BM>::LDS (MOCR_QQT_LDS: more)
};

static int qqt_block_rows(int regime_rows) {
    static const int bm64_rows = env_int("MOCR_QQT_BM64_ROWS", 1280);
    return regime_rows <= bm64_rows ? 64 : 128;
}
// ... and the row count the decode step makes that choice by: the rows the launch has (the block shape does not touch a sum;
// MOCR_NEUTRAL_BY_ROWS=0: the batch's regime)
static int qqt_choice_rows(const mocr_engine* e, int n) {
    static const int neutral_by_rows = env_int("MOCR_NEUTRAL_BY_ROWS", 2);
    return neutral_by_rows ? n : e->rrows(n);
}

void launch_qqt(mocr_engine* e, const QqtParams& q, int n, int regime_rows) {
    const int bm = qqt_block_rows(regime_rows);
    const int lds = bm == 64 ? QqtCfg<64>::LDS : env_int("MOCR_QQT_LDS", QQT_LDS);
    hipLaunchKernelGGL(find_form<QqtFamily>({bm}).kernel, dim3((n + bm - 1) / bm, 12), dim3(256), lds, e->stream, q);
    HIPCHECK(hipGetLastError());
}

// The latent block's query path, by the batch's regime.  dec_use_qqt: q and Qt in one launch (kernels_qqt.h) from 257 rows,
// i.e. for every batch the product decodes on the latent path; dec_qt_tile: the tile of the head-batched Qt GEMM of the
// two-launch path (128 from 1024 rows).  launch_latent_block launches by them and decode_plan reports them.
static bool dec_use_qqt(const mocr_engine* e, int n) {
    // fat batches: q and Qt in one launch (kernels_qqt.h), 37 us instead of 16 + 31 at 4096 rows; bit-identical to the
    // two-launch path.  MOCR_DEC_QQT_ROWS = rows from which it is used (0 = never)
    // (r04, tools/r04_qqt_rows_ab.sh, isolated batch, two launches / fused: 512 rows 136.2 / 134.9 ms, 768 rows 165.4 / 163.5, below
    // 512 rows the two launches stay ahead: the switch moved from 1024 to 512 rows)
    // (r04, 64-row blocks, tools/r04_qqt_rows_ab2.sh, two launches / fused: 288 rows 103.6 / 100.4 ms, 320 rows 105.0 / 101.5, 384 rows
    // 107.7 / 104.6, 448 and 512 rows equal: every latent batch - 257 rows and up - takes the fused launch)
    static const int qqt_rows = env_int("MOCR_DEC_QQT_ROWS", 257);
    return qqt_rows > 0 && e->rrows(n) >= qqt_rows && e->D == 768 && e->H == 12 && !(e->cfg.flags & MOCR_FLAG_NO_FUSED_QQT);
}
static int dec_qt_tile(const mocr_engine* e, int n) {
    static const int qttile_env = env_int("MOCR_DEC_QTTILE", 0);
    return qttile_env ? qttile_env : (e->rrows(n) >= 1024 ? 128 : 64);      // Qt is output-write bound: fewer, fatter blocks
}

// q -> Qt -> latent attention -> ctx: the attention block of the latent path up to (not including)
// the output projection.  wq/bq: query projection; wkT: (Wk^T)/8; wv/bv: value projection.  The choices are made by
// e->rrows(n), the batch's regime.
void launch_latent_block(mocr_engine* e, const LatentBlockArgs& a) {
    using T = bf16_t;
    const int D = e->D, n = a.n;
    auto latent_ctx = [&] {          // ctx = Et Wv^T + bv, one GEMM per head
        HeadBatch hc; hc.heads = e->H; hc.a_yoff = D; hc.w_yoff = (long long)64 * D; hc.o_yoff = 64; hc.b_yoff = 64; hc.ldw = D;
        GemmCall c = gemm_call("gemm_dec_ctx", a.et, 16 * D, a.wv, a.bv, a.ctx, D, n, 64, D, EPI_BIAS, 64);
        c.hb = &hc;
        gemm<T>(e, c);
    };
    if (dec_use_qqt(e, n)) {
        QqtParams q{};
        q.x = reinterpret_cast<const bf16_t*>(a.xin); q.wq = reinterpret_cast<const bf16_t*>(a.wq); q.bq = a.bq;
        q.wkT = reinterpret_cast<const bf16_t*>(a.wkT); q.qt = reinterpret_cast<bf16_t*>(a.qt);
        {
            ProfScope ps(e, "dec_qqt", 4.0 * n * D * D, (double)n * D * 2 + 2.0 * D * D * 2 + (double)n * e->H * D * 2);
            launch_qqt(e, q, n, qqt_choice_rows(e, n));
        }
        latent_attn(e, a);
        latent_ctx();
        return;
    }
    static const int qtile = env_int("MOCR_DEC_QTILE", 64);
    const int qttile = dec_qt_tile(e, n);
    gemm<T>(e, gemm_call("gemm_dec_q", a.xin, D, a.wq, a.bq, a.q, D, n, D, D, EPI_BIAS, qtile));
    HeadBatch hq; hq.heads = e->H; hq.a_yoff = 64; hq.w_yoff = 64; hq.o_yoff = D; hq.b_yoff = 0; hq.ldw = D;
    GemmCall qt = gemm_call("gemm_dec_qt", a.q, D, a.wkT, e->w.zero_bias, a.qt, 16 * D, n, D, 64, EPI_BIAS, qttile);
    qt.hb = &hq;
    gemm<T>(e, qt);
    latent_attn(e, a);
    latent_ctx();
}

// The decode step's latent block of one layer: keys = the layer's cached input rows (self, context t + 1) or the encoder
// output (cross), intermediates in the engine's q / Qt / Et buffers, the result in ctx_t.
LatentBlockArgs latent_block_args(const mocr_engine* e, bool self, int layer, int n, int t, const void* xin, const void* wq,
                                  const float* bq, const void* wkT, const void* wv, const float* bv) {
    LatentBlockArgs a{};
    a.self = self; a.n = n; a.approx_len = self ? t + 1 : e->S;
    a.xin = xin; a.wq = wq; a.bq = bq; a.wkT = wkT; a.wv = wv; a.bv = bv;
    const size_t cache_layer = (size_t)layer * e->Bp * e->cfg.max_len * e->D;     // elements (bytes for e4m3)
    if (e->fp8attn) {
        a.keys = self ? e->x8cache + cache_layer : e->enc8;
        a.sx = self ? e->w.sx_self[layer] : e->w.sx_enc;
    } else {
        a.keys = self ? reinterpret_cast<const bf16_t*>(e->xcache) + cache_layer : reinterpret_cast<const bf16_t*>(e->ENC);
    }
    a.key_stride = self ? (long long)e->cfg.max_len * e->D : (long long)e->S * e->D;
    a.fixed_len = self ? 0 : e->S;
    a.step = self ? e->step : nullptr;
    a.rowmap = e->rowmap;
    a.q = e->q_t; a.qt = e->qt; a.et = e->et; a.ctx = e->ctx_t;
    return a;
}

void latent_block(mocr_engine* e, bool self, int layer, int n, int t, const void* xin, const void* wq, const float* bq,
                  const void* wkT, const void* wv, const float* bv) {
    launch_latent_block(e, latent_block_args(e, self, layer, n, t, xin, wq, bq, wkT, wv, bv));
}

// smallm_gemm_kernel<PRO, EPI, MT, KS> (kernels_smallm.h): the (prologue, epilogue) pairs of the small-batch step x one / two
// 16-row tiles x K = 768 / 3072 (KS = 3 / 12; the LayerNorm prologue has K = 768 only).
struct SmallMArgs { int pro, epi, mt, ks; };
constexpr bool operator==(const SmallMArgs& a, const SmallMArgs& b) { return a.pro == b.pro && a.epi == b.epi && a.mt == b.mt && a.ks == b.ks; }
constexpr std::array<SmallMArgs, 14> smallm_forms() {
    constexpr int pairs[][2] = {{SM_PRO_PLAIN, SM_EPI_RAW}, {SM_PRO_LN, SM_EPI_RAW}, {SM_PRO_PLAIN, SM_EPI_SUM}, {SM_PRO_LN, SM_EPI_GELU_BF16},
                                {SM_PRO_LN, SM_EPI_GELU_F32}};
    std::array<SmallMArgs, 14> a{};
    int n = 0;
    for (const auto& pe : pairs)
        for (int mt : {1, 2})
            for (int ks : {3, 12})
                if (ks == 3 || pe[0] == SM_PRO_PLAIN) a[n++] = SmallMArgs{pe[0], pe[1], mt, ks};
    return a;
}
struct SmallMFamily {
    using Args = SmallMArgs;
    using Kernel = void (*)(SmallMParams);
    static constexpr std::array<Args, 14> forms = smallm_forms();
    static_assert(forms[13].mt == 2, "smallm_forms fills its table");
    template <size_t I> static constexpr Kernel kernel() { constexpr Args a = forms[I]; return smallm_gemm_kernel<a.pro, a.epi, a.mt, a.ks>; }
    static constexpr int lds(const Args& a) { return SM_LDS(a.pro, a.mt); }
};
static bool smallm_pair_exists(int pro, int epi) {
    return std::any_of(SmallMFamily::forms.begin(), SmallMFamily::forms.end(), [&](const SmallMArgs& f) { return f.pro == pro && f.epi == epi; });
}

void smallm_gemm(mocr_engine* e, const char* name, int pro, int epi, SmallMParams p) {
    p.eps = e->cfg.ln_eps;
    const int mt = (p.rows + 15) / 16;
    if (mt < 1 || mt > 2 || p.N % SM_NT || (p.K != 768 && p.K != 3072) || (pro == SM_PRO_LN && p.K != 768))
        throw ArgError{"small-batch GEMM: unsupported shape", MOCR_ERR_UNSUPPORTED};
    const auto f = find_form<SmallMFamily>({pro, epi, mt, p.K / 256});
    if (!f.kernel) throw ArgError{"small-batch GEMM: (pro, epi) is not a pair the small-batch decode step launches", MOCR_ERR_UNSUPPORTED};
    ProfScope ps(e, name, 2.0 * p.rows * p.N * p.K, (double)p.N * p.K * 2);
    hipLaunchKernelGGL(f.kernel, dim3(p.N / SM_NT), dim3(64 * SM_NW), f.lds, e->stream, p);
    HIPCHECK(hipGetLastError());
}

// One greedy step of a SMALL bf16 batch (<= 32 rows, classic attention): 19 launches instead of 28 (kernels_smallm.h).
// x_f32 / a_f32 / c_f32 hold PRE-LayerNorm sums here (s3 of the previous layer - or the embedding rows for layer 0 -,
// s1, s2); ln_stats[k] the (mean, rstd) of s(k+1), published by the first projection that normalises it.
void decode_step_smallm(mocr_engine* e, const DecState& st, const DecMode& m, int n, int t) {
    using T = bf16_t;
    const int D = e->D, F = e->F;
    auto& w = e->w;
    float* const st1 = e->ln_stats, * const st2 = e->ln_stats + 2 * e->Bp, * const st3 = e->ln_stats + 4 * e->Bp;
    auto W = [](const void* q) { return reinterpret_cast<const bf16_t*>(q); };
    for (int l = 0; l < e->cfg.dec_layers; ++l) {
        const DecLayerW& L = w.dec[l];
        const DecLayerW* P = l ? &w.dec[l - 1] : nullptr;        // the layer whose LayerNorm 3 produces this layer's input
        SmallMParams q{};
        q.rows = n; q.K = D; q.w = W(L.wqkv); q.N = 3 * D; q.out = e->slabs; q.ldo = 3 * D;
        if (!P) { q.a_bf16 = W(e->x_t); smallm_gemm(e, "sm_qkv", SM_PRO_PLAIN, SM_EPI_RAW, q); }
        else { q.a_f32 = e->x_f32; q.ln_g = P->ln3g; q.ln_b = P->ln3b; q.stats_out = st3; smallm_gemm(e, "sm_qkv", SM_PRO_LN, SM_EPI_RAW, q); }
        dec_attn<T, true>(e, l, 1, n, L.bqkv, t + 1);
        SmallMParams o{};
        o.rows = n; o.K = D; o.a_bf16 = W(e->ctx_t); o.w = W(L.wo); o.N = D; o.bias = L.bo; o.out = e->a_f32; o.ldo = D;
        o.resid = e->x_f32;
        if (P) { o.resid_stats = st3; o.resid_g = P->ln3g; o.resid_b = P->ln3b; }
        smallm_gemm(e, "sm_proj", SM_PRO_PLAIN, SM_EPI_SUM, o);                       // s1 = ctx Wo^T + bo + layer input
        SmallMParams c{};
        c.rows = n; c.K = D; c.a_f32 = e->a_f32; c.ln_g = L.ln1g; c.ln_b = L.ln1b; c.stats_out = st1;
        c.w = W(L.wqc); c.N = D; c.out = e->slabs; c.ldo = D;
        smallm_gemm(e, "sm_qc", SM_PRO_LN, SM_EPI_RAW, c);
        if (m.positions && l + 1 == e->cfg.dec_layers) {      // token positions: the rows sm_qc's prologue normalised, recorded
            ProfScope ps(e, "pos_hist_ln", 0, (double)n * D * 6);
            hipLaunchKernelGGL((hist_ln_rows_kernel<T>), dim3((n + 15) / 16), dim3(256), 0, e->stream, (const float*)e->a_f32, (const float*)L.ln1g,
                               (const float*)L.ln1b, e->cfg.ln_eps, reinterpret_cast<T*>(e->pos_hist), (long long)st.max_len * D,
                               (const int*)e->step, (const int*)e->rowmap, n);
            HIPCHECK(hipGetLastError());
        }
        dec_attn<T, false>(e, l, 1, n, L.bqc, e->S);
        SmallMParams oc{};
        oc.rows = n; oc.K = D; oc.a_bf16 = W(e->ctx_t); oc.w = W(L.woc); oc.N = D; oc.bias = L.boc; oc.out = e->c_f32; oc.ldo = D;
        oc.resid = e->a_f32; oc.resid_stats = st1; oc.resid_g = L.ln1g; oc.resid_b = L.ln1b;
        smallm_gemm(e, "sm_proj", SM_PRO_PLAIN, SM_EPI_SUM, oc);                      // s2 = ctx Woc^T + boc + LN1(s1)
        SmallMParams f1{};
        f1.rows = n; f1.K = D; f1.a_f32 = e->c_f32; f1.ln_g = L.ln2g; f1.ln_b = L.ln2b; f1.stats_out = st2;
        f1.w = W(L.w1); f1.N = F; f1.bias = L.b1; f1.out = e->h_t; f1.ldo = F;
        smallm_gemm(e, "sm_fc1", SM_PRO_LN, SM_EPI_GELU_BF16, f1);
        SmallMParams f2{};
        f2.rows = n; f2.K = F; f2.a_bf16 = W(e->h_t); f2.w = W(L.w2); f2.N = D; f2.bias = L.b2; f2.out = e->x_f32; f2.ldo = D;
        f2.resid = e->c_f32; f2.resid_stats = st2; f2.resid_g = L.ln2g; f2.resid_b = L.ln2b;
        smallm_gemm(e, "sm_fc2", SM_PRO_PLAIN, SM_EPI_SUM, f2);                       // s3 = h W2^T + b2 + LN2(s2)
    }
    const DecLayerW& Z = w.dec[e->cfg.dec_layers - 1];
    SmallMParams tr{};
    tr.rows = n; tr.K = D; tr.a_f32 = e->x_f32; tr.ln_g = Z.ln3g; tr.ln_b = Z.ln3b;
    tr.w = W(w.wt); tr.N = D; tr.bias = w.bt; tr.out = e->a_f32; tr.ldo = D;
    smallm_gemm(e, "sm_transform", SM_PRO_LN, SM_EPI_GELU_F32, tr);                   // gelu(LN3(s3) Wt^T + bt), pre-LayerNorm
    SmallMParams v{};
    v.rows = n; v.K = D; v.a_f32 = e->a_f32; v.ln_g = w.lntg; v.ln_b = w.lntb;
    v.w = W(w.wv); v.N = e->V; v.out = e->slabs; v.ldo = e->V;
    smallm_gemm(e, "sm_vocab", SM_PRO_LN, SM_EPI_RAW, v);
    dec_token<T, false>(e, st, m, 1, n);
}

// One greedy step for n rows; `t` is only used for the profiler's byte estimate.
template <typename T>
void decode_step(mocr_engine* e, const DecState& st, const DecMode& m, int n, int t) {
    if constexpr (sizeof(T) == 2) {
        if (!m.beam && e->use_smallm(e->rrows(n))) { decode_step_smallm(e, st, m, n, t); return; }
    }
    const int D = e->D, F = e->F;
    auto& w = e->w;
    const void* xin = e->x_t;
    const float* xres = e->x_f32;
    const int rn = e->rrows(n);          // the row count the kernel choices are made by (the batch's regime)
    for (int l = 0; l < e->cfg.dec_layers; ++l) {
        const DecLayerW& L = w.dec[l];
        int ns;
        const size_t esz = sizeof(T);
        if (e->use_latent(rn)) {
            latent_block(e, true, l, n, t, xin, L.wqkv, L.bqkv, L.wkT_s, reinterpret_cast<const char*>(L.wqkv) + (size_t)2 * D * D * esz,
                         L.bqkv + 2 * D);
        } else {
            ns = dec_gemm<T>(e, "gemm_dec_qkv", xin, D, L.wqkv, 3 * D, D, n);
            dec_attn<T, true>(e, l, ns, n, L.bqkv, t + 1);   // t = step index = keys already cached
        }
        ns = dec_gemm<T>(e, "gemm_dec_proj", e->ctx_t, D, L.wo, D, D, n);
        // (token positions: the last layer's LayerNorm-1 rows are also recorded, at the input token's position step[slot])
        dec_add_ln<T>(e, ns, D, L.bo, xres, L.ln1g, L.ln1b, e->a_f32, e->a_t, n, false, -1,
                      (m.positions && l + 1 == e->cfg.dec_layers) ? e->pos_hist : nullptr, st.max_len);
        if (e->use_latent(rn)) {
            latent_block(e, false, l, n, t, e->a_t, L.wqc, L.bqc, L.wkT_c,
                         reinterpret_cast<const char*>(w.wckv) + (size_t)(2 * l + 1) * D * D * esz, w.bckv + (2 * l + 1) * D);
        } else {
            ns = dec_gemm<T>(e, "gemm_dec_proj", e->a_t, D, L.wqc, D, D, n);
            dec_attn<T, false>(e, l, ns, n, L.bqc, e->S);
        }
        ns = dec_gemm<T>(e, "gemm_dec_proj", e->ctx_t, D, L.woc, D, D, n);
        dec_add_ln<T>(e, ns, D, L.boc, e->a_f32, L.ln2g, L.ln2b, e->c_f32, e->c_t, n, false);
        if (dec_fc1_fused<T>(e, n)) {
            gemm<T>(e, gemm_call("gemm_dec_fc1", e->c_t, D, L.w1, L.b1, e->h_t, F, n, F, D, EPI_BIAS_GELU, dec_launch_tile(e, n)));
        } else {
            ns = dec_gemm<T>(e, "gemm_dec_fc1", e->c_t, D, L.w1, F, D, n);
            launch_dec_bias_gelu<T>(e, e->slabs, ns, (long long)e->Bp * F, L.b1, e->h_t, n, F);
        }
        ns = dec_gemm<T>(e, "gemm_dec_fc2", e->h_t, F, L.w2, D, F, n);
        dec_add_ln<T>(e, ns, D, L.b2, e->c_f32, L.ln3g, L.ln3b, e->x_f32, e->x_t, n, false,
                      (e->use_latent(rn) && l + 1 < e->cfg.dec_layers) ? l + 1 : -1);
        xin = e->x_t; xres = e->x_f32;
    }
    int ns = dec_gemm<T>(e, "gemm_dec_proj", e->x_t, D, w.wt, D, D, n);
    dec_add_ln<T>(e, ns, D, w.bt, nullptr, w.lntg, w.lntb, nullptr, e->z_t, n, true);
    // LM head.  When the GEMM is not split over K and nobody asked for the logits, its epilogue reduces every N-tile
    // to (max, column) and the token kernel picks among V/tile candidates: the [n, V] fp32 logits (100 MB at 4096
    // rows) are neither written nor read.  acc + bias is the same fp32 value either way, so the argmax is identical.
    if (m.beam) {       // beam search: the selection needs whole rows - always the slab form of the LM head
        ns = dec_gemm<T>(e, "gemm_dec_vocab", e->z_t, D, w.wv, e->V, D, n);
        beam_finish_step<T>(e, st, m, ns, n, t);
        return;
    }
    const int vt = dec_launch_tile(e, n);
    if (!st.logits_out && dec_head_fused<T>(e, n)) {
        // (a scored batch also keeps every tile's sum of exp(logit - tile max): EPI_ARGMAX_LSE, same max / column; an
        // alternatives batch every tile's four best as well: EPI_TOPK; a constrained batch the masked form of either: EPI_*_M)
        LmHead lm;
        lm.cand_idx = e->cand_idx;
        if (m.level >= 1) lm.cand_sum = e->cand_sum;
        if (m.level >= 2) { lm.top_val = e->top_val; lm.top_idx = e->top_idx; }
        if (m.mask) lm.mask = TokMask{st.tok_mask, st.set_of_row, st.rowmap};
        if (m.prefix) lm.target = TokTarget{st.prefix, st.prefix_len, st.prefix_ld, st.step, e->tgt_val};
        if (m.soft) lm.soft = TokSoft{e->aut_state, e->aut_edge_begin, e->aut_edge_token, e->aut_edge_weight};
        if (m.penalty) lm.pen = TokPen{e->seen_mask, e->penalty_of_row};
        GemmCall head = gemm_call(m.head_name(), e->z_t, D, w.wv, w.bv, e->cand_val, e->V, n, e->V, D, m.epilogue(), vt);
        head.lm = &lm;
        gemm<T>(e, head);
        dec_token<T, false>(e, st, m, 1, n, e->V / vt);
    } else {
        ns = dec_gemm<T>(e, "gemm_dec_vocab", e->z_t, D, w.wv, e->V, D, n);
        dec_token<T, false>(e, st, m, ns, n);
    }
}

template <typename T>
void run_cross_kv(mocr_engine* e, int n) {
    const int M = n * e->S;
    static const int enc_tile_env = env_int("MOCR_ENC_TILE", 0);
    const bool few_blocks = (long long)((M + 127) / 128) * (e->NCKV / 128) * 5 <= 4LL * e->num_cus;      // see run_encoder
    const bool big = sizeof(T) == 2 && (long long)((M + 255) / 256) * (e->NCKV / 256) >= e->num_cus && e->NCKV % 256 == 0;
    const int ET = enc_tile_env ? enc_tile_env : big ? TILE_PERSISTENT : few_blocks ? 64 : 128;
    gemm<T>(e, gemm_call("gemm_cross_kv", e->ENC, e->D, e->w.wckv, e->w.bckv, e->CKV, e->NCKV, M, e->NCKV, e->D, EPI_BIAS, ET));
}

// fp8 attention: the batch's encoder output as e4m3 rows (static scale), once per batch
void quantize_enc(mocr_engine* e, int n) {
    const long long n16 = (long long)n * e->S * e->D / 16;
    ProfScope ps(e, "quant_enc_fp8", 0, (double)n * e->S * e->D * 3);
    hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, e->stream,
                       reinterpret_cast<const bf16_t*>(e->ENC), e->enc8, n16, 1.0f / e->w.sx_enc);
    HIPCHECK(hipGetLastError());
}

// Raise the dynamic-LDS limit of every form of every kernel family (done once, at creation: outside any capture, from the
// calling thread - decode steps are launched inside stream capture and from several lane threads).
template <typename T> void init_kernel_attrs() {
    raise_lds<TileFamily<T>, PersFamily, QqtFamily, SmallMFamily, LatentFamily, LatentTFamily, Latent8Family, LatentT8Family>();
    for_each_enc_attn<T>([](auto kernel, int lds) { set_max_lds(kernel, lds); });
#ifdef MOCR_EXPERIMENTS
    raise_lds<Gemm256Family, WideFamily, Wide2Family>();
#endif
}

// `steps` consecutive greedy steps captured once and replayed: every per-step value (position,
// token, finished flags) lives in device memory, so the launch sequence is identical each step.
template <typename T>
hipGraphExec_t decode_graph(mocr_engine* e, const DecState& st, const DecMode& m, int n, int steps, int t0) {
    // the self-attention variant depends on the context length, so graphs are bucketed by it
    const int need = ((t0 + steps + 3) / 4 + 7) / 8;
    const int bucket = need <= 3 ? 3 : need <= 5 ? 5 : need <= 8 ? 8 : 10;
    const int t_hi = std::min(bucket * 32, st.max_len) - 1;      // largest context this bucket covers
    // ... and by the mode of the steps: another LM-head epilogue, token kernel, set of pointers or launch each
    long long beam_key = 0;          // a beam batch: which configuration the captured launches carry (1-based, above the mode bits)
    if (m.beam) {
        auto& cfgs = e->beam_cfgs;
        size_t i = 0;
        while (i < cfgs.size() && !same_beam(cfgs[i], m.beam_cfg)) ++i;
        if (i == cfgs.size()) {
            if (i >= 100) throw ArgError{"more than 100 distinct beam configurations on one engine", MOCR_ERR_UNSUPPORTED};
            cfgs.push_back(m.beam_cfg);
        }
        beam_key = ((long long)i + 1) << 32;
    }
    const auto key = std::make_tuple(e->lane_id, n, (long long)(st.max_len * 16 + bucket) * DecMode::KEY_SPAN + m.key_bits() + beam_key, steps, e->rrows(n));
    auto it = e->graphs.find(key);
    if (it != e->graphs.end()) return it->second;
    hipGraph_t g = nullptr;
    HIPCHECK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    try {
        for (int i = 0; i < steps; ++i) decode_step<T>(e, st, m, n, t_hi - 1);
    } catch (...) {
        (void)hipStreamEndCapture(e->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    HIPCHECK(hipStreamEndCapture(e->stream, &g));
    hipGraphExec_t ge = nullptr;
    HIPCHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    HIPCHECK(hipGraphDestroy(g));
    e->graphs[key] = ge;
    return ge;
}

// Teacher-forced decode (test hook): eager launches, logits of every step kept.
template <typename T>
void run_decode_forced(mocr_engine* e, int n, const int* forced, int forced_T, float* logits_out) {
    DecState st = make_state(e, e->cfg.max_len, forced, forced_T, logits_out, n);
    dec_token<T, true>(e, st, DecMode{}, 0, n);
    for (int t = 0; t < forced_T; ++t) decode_step<T>(e, st, DecMode{}, n, t);
}

// ---------------------------------------------------------------------------------------- scheduler
// A job moves through: start (input staging, encoder, cross-K/V, start token) -> chunks of CHUNK
// greedy steps (one HIP-graph replay each) -> finish (copy ids/lengths out).  After each chunk the
// lane's unfinished-row counter is copied to pinned memory; the flag of chunk c-2 is examined
// before chunk c is enqueued, so a lane always has work queued while the host looks at a flag, and
// a batch whose rows have all emitted EOS stops at most one chunk late.
constexpr int CHUNK = 8;
// Small batches use shorter chunks: their steps are launch-bound (105-165 us whatever the rows), a batch whose rows have
// all finished is noticed (c_f + 2) chunks in, and ordinary speech-bubble texts are 10-30 tokens.  Measured (r02,
// tools/short_text_probe.py, <= 16 rows, every row ending at once): 8-step chunks 3.03 ms, 4-step 2.19 ms, 2-step
// 1.71 ms, i.e. a 20-token batch 4.9 -> 3.9 ms; long rows are unaffected up to 16 rows (106 tokens alone: 14.4 -> 13.7 ms),
// while at 64 rows 2-step chunks cost +3 % on 300-token rows and 4-step chunks nothing.  A replay costs the host
// 10-16 us against >= 210 us of GPU work per chunk.  MOCR_SMALL_CHUNK (with MOCR_SMALL_CHUNK_ROWS): experiments.
static int chunk_steps(int rows) {
    static const int forced = env_int("MOCR_SMALL_CHUNK", 0), forced_rows = env_int("MOCR_SMALL_CHUNK_ROWS", 128);
    if (forced > 0) return rows <= forced_rows ? std::min(forced, CHUNK) : CHUNK;
    return rows <= 16 ? 2 : rows <= 128 ? 4 : CHUNK;
}

// Decode graphs are keyed by row count.  Callers submit any n in 1..max_batch (the batcher of MangaOcr, the crop-job
// queue), so n is rounded up to a coarse grid before it becomes a key: at most ~50 distinct row counts per engine
// instead of max_batch, i.e. a bounded number of captures / instantiated graphs, and a batch of 37 crops replays the
// graph a batch of 40 captured.  The padding costs <= 12.5 % more rows in the (latency-bound) decode steps.
static int graph_rows(int n, int max_batch) {
    int q;
    if (n <= 8) q = 1;
    else if (n <= 64) q = 8;
    else if (n <= 256) q = 32;
    else if (n <= 1024) {
        // (r04: 64 instead of 128 - a 288-row batch decoded on 384 slots.  tools/r04_graphq_ab.sh, isolated batches, 128 / 64:
        // 272-320 rows 100-102 / 95-97 ms, 416-448 rows 113-116 / 109-111, 544 rows 128.6 / 126.6, 700 rows 148 / 145)
        static const int q_mid = env_int("MOCR_GRAPH_Q_MID", 64);
        q = q_mid;
    }
    else q = 256;       // (r04: 512 until rows were compacted - a batch now passes through these row counts on its way down)
    return std::min(round_up(n, q), max_batch);
}

// What a greedy decode step of `rows` rows decides (the batch's regime is e->regime, 0 = rows) - from the helpers the step
// itself launches through: use_smallm / use_latent, dec_tile / dec_launch_tile, dec_split (pick_split), dec_fc1_fused,
// dec_head_fused, tile_launch (the ring), dec_use_qqt, qqt_block_rows, dec_qt_tile, dec_attn_nt, chunk_steps, graph_rows.
// Nothing is launched and rows need not fit max_batch; mocr_decode_plan reports it.  The five GEMM entries say how the tile
// kernel is launched for that shape at these rows whether or not this engine's path launches it (the small-batch path
// launches none of them, the latent path no QKV GEMM): they depend on the dtype, the CUs and the flags, not on max_batch.
struct DecGemmPlan { int split, ring, epi; };     // K slices, ring slots (2 / 4), epilogue (EPI_SLAB, EPI_BIAS_GELU, EPI_ARGMAX)
struct DecPlan {
    int path;                         // 0 small-batch (kernels_smallm.h), 1 classic attention, 2 latent attention
    int regime_tile, launch_tile;     // the tile the split is chosen for (the regime's) / the tile the GEMMs are launched on
    DecGemmPlan g[5];                 // QKV 2304 x 768, projections 768 x 768, FC1 3072 x 768, FC2 768 x 3072, vocabulary V x 768
    bool qkv_tile_gemm;               // the step launches QKV as a tile GEMM (classic path only)
    bool qqt; int qqt_bm;             // latent path: q and Qt in one launch, and its rows per block (0: two launches)
    int qt_tile;                      // latent path, two launches: the Qt GEMM's tile (0: not launched)
    bool attn_nt;                     // classic attention: non-temporal K/V loads
    int chunk, graph_rows;            // steps per graph replay; the rows this count is rounded up to (<= max_batch)
};
// The only writer of mocr_engine::regime: set around a batch's scheduling step (pump_once) or a test hook's launches (or its
// plan), and put back on every way out - an exception too
struct RegimeScope {
    mocr_engine* e; int old;
    RegimeScope(mocr_engine* e_, int r) : e(e_), old(e_->regime) { e->regime = r; }
    ~RegimeScope() { e->regime = old; }
};
template <typename T>
DecPlan decode_plan(const mocr_engine* e, int rows) {
    const int D = e->D, F = e->F, V = e->V, kt = 128 / (int)sizeof(T), rn = e->rrows(rows);
    DecPlan pl{};
    pl.path = (sizeof(T) == 2 && e->use_smallm(rn)) ? 0 : e->use_latent(rn) ? 2 : 1;
    pl.regime_tile = dec_tile(rn);
    pl.launch_tile = dec_launch_tile(e, rows);
    auto launched = [&](int N, int K, int split, int epi) {
        return DecGemmPlan{split, tile_launch(e, rows, N, pl.launch_tile, split, 1, K / split / kt).ring, epi};
    };
    auto slabs = [&](int N, int K) { return launched(N, K, dec_split<T>(e, N, K, rows), EPI_SLAB); };
    pl.g[0] = slabs(3 * D, D);
    pl.g[1] = slabs(D, D);
    pl.g[2] = dec_fc1_fused<T>(e, rows) ? launched(F, D, 1, EPI_BIAS_GELU) : slabs(F, D);
    pl.g[3] = slabs(D, F);
    pl.g[4] = dec_head_fused<T>(e, rows) ? launched(V, D, 1, EPI_ARGMAX) : slabs(V, D);
    pl.qkv_tile_gemm = pl.path == 1;
    pl.qqt = pl.path == 2 && dec_use_qqt(e, rows);
    pl.qqt_bm = pl.qqt ? qqt_block_rows(qqt_choice_rows(e, rows)) : 0;
    pl.qt_tile = (pl.path == 2 && !pl.qqt) ? dec_qt_tile(e, rows) : 0;
    pl.attn_nt = pl.path != 2 && dec_attn_nt(e, rows);
    pl.chunk = chunk_steps(rows);
    pl.graph_rows = graph_rows(rows, e->cfg.max_batch);
    return pl;
}

// The buffers of the token alternatives, for the bound lane: allocated by the first batch that needs them (under the engine
// lock like every scheduling step, and never inside a graph capture: start_batch captures nothing), so an engine that is
// never asked keeps the memory footprint it had - default_max_batch sizes batches from the free HBM.
static void ensure_alt_buffers(mocr_engine* e) {
    if (e->alt_ids) return;
    const size_t Bp = (size_t)e->Bp;
    e->top_val = e->dalloc<float>(Bp * (e->V / 64) * MOCR_ALTERNATIVES); e->top_idx = e->dalloc<int>(Bp * (e->V / 64) * MOCR_ALTERNATIVES);
    e->alt_logp = e->dalloc<float>(Bp * e->cfg.max_len * MOCR_ALTERNATIVES);
    e->alt_ids = e->dalloc<int>(Bp * e->cfg.max_len * MOCR_ALTERNATIVES);
}

// The set of every row of a constrained batch, for the bound lane: allocated by the first constrained batch, like the
// alternatives buffers.
static void ensure_set_buffer(mocr_engine* e) {
    if (!e->set_of_row) e->set_of_row = e->dalloc<int>((size_t)e->Bp);
}

// The device table of the token sets, row 0 (MOCR_TOKEN_SET_ALL) all ones: allocated by the first set or the first batch with
// no-repeat n-grams, whose rows' base sets are rows of it.
static void ensure_tok_table(mocr_engine* e) {
    if (e->tok_table) return;
    const size_t words = (size_t)e->V / 32;
    e->tok_table = e->dalloc<unsigned>((size_t)MOCR_MAX_TOKEN_SETS * words);
    e->tok_sets.push_back(std::vector<uint32_t>(words, 0xffffffffu));        // set 0: the whole vocabulary
    e->tok_index[e->tok_sets[0]] = MOCR_TOKEN_SET_ALL;
    HIPCHECK(hipMemcpy(e->tok_table, e->tok_sets[0].data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
}

// The per-row masks of the no-repeat n-grams, for the bound lane: allocated by the first batch that has a row with n > 0, like
// the alternatives buffers (768 B a row).
static void ensure_ngram_buffers(mocr_engine* e) {
    if (e->row_mask) return;
    const size_t Bp = (size_t)e->Bp;
    e->row_mask = e->dalloc<unsigned>(Bp * (e->V / 32));
    e->ngram_of_row = e->dalloc<int>(Bp);
    e->row_ident = e->dalloc<int>(Bp);
    std::vector<int> ident(Bp);
    for (size_t i = 0; i < Bp; ++i) ident[i] = (int)i;
    HIPCHECK(hipMemcpy(e->row_ident, ident.data(), Bp * sizeof(int), hipMemcpyHostToDevice));
}

// The rows' forced prefixes and the slots' target values, for the bound lane: allocated by the first batch that has a
// prefix, like the alternatives buffers.
static void ensure_prefix_buffers(mocr_engine* e) {
    if (e->prefix) return;
    const size_t Bp = (size_t)e->Bp;
    e->prefix = e->dalloc<int>(Bp * e->cfg.max_len);
    e->prefix_len = e->dalloc<int>(Bp);
    e->tgt_val = e->dalloc<float>(Bp);
}

static void launch_ngram_init(mocr_engine* e, unsigned* row_mask, const unsigned* base_mask, const int* base_set_of_row,
                              const int* ngram_of_row, int rows) {
    ProfScope ps(e, "ngram_init", 0, (double)rows * (e->V / 32) * 8);
    hipLaunchKernelGGL(ngram_init_kernel, dim3(rows), dim3(192), 0, e->stream, row_mask, base_mask, base_set_of_row, ngram_of_row, rows,
                       e->V / 32, e->cfg.start_id);
    HIPCHECK(hipGetLastError());
}

// ---- token automata --------------------------------------------------------------
constexpr size_t AUT_ARENA_BYTES = ((size_t)MOCR_MAX_AUTOMATON_STATES + 1) * sizeof(int) + 2 * (size_t)MOCR_MAX_AUTOMATON_EDGES * sizeof(int) +
                                   (size_t)MOCR_MAX_AUTOMATON_STATES;

// The device arena of the automata, allocated once at full capacity by the first mocr_automaton_create (about 37 MiB): the
// captured decode graphs hold its addresses, so it never grows or moves.
static void ensure_automaton_arena(mocr_engine* e) {
    if (e->aut_edge_begin) return;
    e->aut_edge_begin = e->dalloc<int>((size_t)MOCR_MAX_AUTOMATON_STATES + 1);
    e->aut_edge_token = e->dalloc<int>((size_t)MOCR_MAX_AUTOMATON_EDGES);
    e->aut_edge_next = e->dalloc<int>((size_t)MOCR_MAX_AUTOMATON_EDGES);
    e->aut_accepting = e->dalloc<uint8_t>((size_t)MOCR_MAX_AUTOMATON_STATES);
}

// The arena's soft part: edge_weight [2^22] and default_next [2^20], 20 MiB, allocated at full capacity by the
// first create of a soft automaton and filled with 0 / -1 - what every automaton that exists or comes later without the two
// arrays reads there.  Nothing has been launched on them yet, so the fill races with nothing.
constexpr size_t AUT_SOFT_ARENA_BYTES = (size_t)MOCR_MAX_AUTOMATON_EDGES * sizeof(float) + (size_t)MOCR_MAX_AUTOMATON_STATES * sizeof(int);
static void ensure_soft_arena(mocr_engine* e) {
    if (e->aut_edge_weight) return;
    float* w = e->dalloc<float>((size_t)MOCR_MAX_AUTOMATON_EDGES);
    int* d = e->dalloc<int>((size_t)MOCR_MAX_AUTOMATON_STATES);
    HIPCHECK(hipMemset(w, 0, (size_t)MOCR_MAX_AUTOMATON_EDGES * sizeof(float)));
    HIPCHECK(hipMemset(d, 0xFF, (size_t)MOCR_MAX_AUTOMATON_STATES * sizeof(int)));
    e->aut_edge_weight = w; e->aut_default_next = d;
}

// The rows' start states and current states, for the bound lane: allocated by the first batch in which a row brings an
// automaton, like the alternatives buffers (12 B a row).
static void ensure_automaton_buffers(mocr_engine* e) {
    if (e->aut_state) return;
    const size_t Bp = (size_t)e->Bp;
    e->aut_base_of_row = e->dalloc<int>(Bp);
    e->aut_state = e->dalloc<int>(Bp);
    e->aut_state_out = e->dalloc<int>(Bp);
}

static void launch_automaton_init(mocr_engine* e, unsigned* row_mask, const unsigned* base_mask, const int* base_set_of_row,
                                  const int* ngram_of_row, int rows, const int* edge_begin, const int* edge_token,
                                  const uint8_t* accepting, const int* aut_base_of_row, int* aut_state,
                                  const int* default_next = nullptr) {
    ProfScope ps(e, default_next ? "automaton_init_sw" : "automaton_init", 0, (double)rows * (e->V / 32) * 8);
    // (soft token automata: the start state may be open; the hard form never reads default_next)
    hipLaunchKernelGGL(default_next ? automaton_init_kernel<true> : automaton_init_kernel<false>, dim3(rows), dim3(192), 0, e->stream, row_mask,
                       base_mask, base_set_of_row, ngram_of_row, rows, e->V / 32, e->cfg.start_id, e->cfg.eos_id, edge_begin, edge_token,
                       accepting, aut_base_of_row, aut_state, default_next);
    HIPCHECK(hipGetLastError());
}

// ---- repetition penalty ----------------------------------------------------------
// The rows' seen words and penalties, for the bound lane: allocated by the first batch that has a row with p != 1, like the
// n-gram masks (772 B a row).
static void ensure_penalty_buffers(mocr_engine* e) {
    if (e->seen_mask) return;
    const size_t Bp = (size_t)e->Bp;
    e->seen_mask = e->dalloc<unsigned>(Bp * (e->V / 32));
    e->penalty_of_row = e->dalloc<float>(Bp);
}

static void launch_penalty_init(mocr_engine* e, unsigned* seen_mask, int rows) {
    ProfScope ps(e, "penalty_init", 0, (double)rows * (e->V / 32) * 4);
    hipLaunchKernelGGL(penalty_init_kernel, dim3(rows), dim3(192), 0, e->stream, seen_mask, rows, e->V / 32, e->cfg.start_id);
    HIPCHECK(hipGetLastError());
}

// ---- token positions --------------------------------------------------------------
// The deferred pass walks a batch's rows in chunks whose query and key scratch stays under this many bytes whatever
// max_batch is (one row needs (197 + max_len) x 768 elements: 87 rows a chunk in bf16 at max_len 300, 43 in fp32).
constexpr size_t POS_SCRATCH_BYTES = (size_t)64 << 20;
static int pos_chunk_rows(const mocr_engine* e) {
    const size_t per_row = (size_t)(e->S + e->cfg.max_len) * e->D * e->esz;
    return (int)std::max<size_t>(1, POS_SCRATCH_BYTES / per_row);
}

// The buffers of the token positions, for the bound lane: allocated by the first batch that asks, like the alternatives
// buffers.  The recorded rows end with one GEMM tile of slack: gemm_kernel reads whole 128-row tiles of its A operand.
static void ensure_pos_buffers(mocr_engine* e) {
    if (e->pos_hist) return;
    const size_t Bp = (size_t)e->Bp, ML = (size_t)e->cfg.max_len, D = (size_t)e->D, R = (size_t)pos_chunk_rows(e);
    e->pos_hist = e->dalloc<char>((Bp * ML + 128) * D * e->esz);
    e->pos_out = e->dalloc<float>(Bp * ML * MOCR_POSITION_FIELDS);
    e->pos_q = e->dalloc<char>(R * ML * D * e->esz);
    e->pos_k = e->dalloc<char>(R * (size_t)e->S * D * e->esz);
}

// The positions kernel on the caller's buffers (kernels_positions.h PosParams): the deferred pass and the operator hook.
template <typename T>
void launch_attn_positions(mocr_engine* e, const PosParams& p, int rows) {
    if (e->S != POS_KEYS || e->D != 768 || e->H != 12 || e->G != 14)
        throw ArgError{"token positions: a 14 x 14 patch grid, 12 heads of 64 only", MOCR_ERR_UNSUPPORTED};
    // the gathered-query form reads the queries of a row's whole group of K, and entry p + 1 <= T of its trail
    if (p.trail && (p.K < 1 || p.K > MOCR_MAX_BEAMS || rows % p.K || p.trail_ld < (long long)p.T + 1))
        throw ArgError{"token positions: the gathered form takes whole groups of K <= 4 rows and a trail of T + 1 entries", MOCR_ERR_ARG};
    if (rows < 1 || p.T < 1) return;
    ProfScope ps(e, "attn_positions", 2.0 * rows * p.T * POS_KEYS * 768, ((double)rows * POS_KEYS + (double)rows * p.T) * 768 * sizeof(T));
    hipLaunchKernelGGL((attn_positions_kernel<T>), dim3((p.T + 15) / 16, rows), dim3(64), 0, e->stream, p);
    HIPCHECK(hipGetLastError());
}

// The deferred pass of a finished batch, on its lane's stream: per chunk of rows the layer's keys K = ENC Wk^T + bk (the latent
// path never builds CKV, so every path computes them here) and queries q = hist Wq^T + bq, both on gemm_kernel, then the
// positions kernel.  Row r's recorded position p holds the step that emitted token p + 1: the outputs start one position in.
// A beam batch: the rows of the outputs are the finished hypotheses - their lengths, and their queries
// gathered through hyp_trail from the rows that ran their steps, which lie in the same chunk: chunks are whole groups of K.
template <typename T>
void run_positions(mocr_engine* e, Lane& L) {
    // (HL: the batch's generate(max_length) - its rows were recorded HL positions apart, so the query GEMM covers no more than
    // the positions the batch could reach; which of them a row did reach is known on the device only)
    const int D = e->D, ML = e->cfg.max_len, HL = L.max_len, S = e->S, l = e->cfg.dec_layers - 1;
    const DecLayerW& W = e->w.dec[l];
    const char* const wk = reinterpret_cast<const char*>(e->w.wckv) + (size_t)(2 * l) * D * D * sizeof(T);
    const float* const bk = e->w.bckv + (size_t)(2 * l) * D;
    const bool beam = L.mode.beam;
    const int K = beam ? L.mode.beam_cfg.num_beams : 1;
    const int R = pos_chunk_rows(e) / K * K;
    if (R < K) throw ArgError{"token positions: the scratch of the deferred pass holds no whole beam group", MOCR_ERR_UNSUPPORTED};
    for (int r0 = 0; r0 < L.n; r0 += R) {
        const int rows = std::min(R, L.n - r0);
        gemm<T>(e, gemm_call("gemm_pos_k", reinterpret_cast<const char*>(e->ENC) + (size_t)r0 * S * D * sizeof(T), D, wk, bk, e->pos_k, D,
                             rows * S, D, D, EPI_BIAS, 128));
        gemm<T>(e, gemm_call("gemm_pos_q", reinterpret_cast<const char*>(e->pos_hist) + (size_t)r0 * HL * D * sizeof(T), D, W.wqc, W.bqc,
                             e->pos_q, D, rows * HL, D, D, EPI_BIAS, 128));
        PosParams p{};
        p.q = e->pos_q; p.q_row_stride = (long long)HL * D;
        p.k = e->pos_k; p.k_row_stride = (long long)S * D;
        p.len = (beam ? e->hyp_len : e->len) + r0; p.len_bias = -1; p.T = L.max_len - 1;
        if (beam) { p.trail = e->hyp_trail + (size_t)r0 * ML; p.trail_ld = ML; p.K = K; }
        p.out_pos = e->pos_out + ((size_t)r0 * ML + 1) * MOCR_POSITION_FIELDS; p.pos_row_stride = (long long)ML * MOCR_POSITION_FIELDS;
        launch_attn_positions<T>(e, p, rows);
    }
}

// THE merge of a per-row array of the batch's jobs: `ld` elements a row over the np slots, in row order, staged in `stage` (the
// lane's: it outlives the async copy) and uploaded to d_dst.  put(job, dst) writes the job's rows at dst, its first row; what
// it leaves alone - the padding rows, a job without the array - reads `fill`.
template <typename V, typename Put>
static void upload_rows(mocr_engine* e, const Lane& L, std::vector<V>& stage, V fill, V* d_dst, Put put, size_t ld = 1) {
    stage.assign((size_t)L.np * ld, fill);
    size_t r0 = 0;
    for (const Job& j : L.jobs) {
        put(j, stage.data() + r0 * ld);
        r0 += j.n;
    }
    HIPCHECK(hipMemcpyAsync(d_dst, stage.data(), stage.size() * sizeof(V), hipMemcpyHostToDevice, e->stream));
}
// put: a job's array as it comes, one element a row (empty: the job has none)
template <typename V> static auto whole(std::vector<V> Job::*field) {
    return [field](const Job& j, V* dst) { std::copy((j.*field).begin(), (j.*field).end(), dst); };
}

// Token constraints: the merged rows' sets (a beam batch: by row c K + k - a beam job carries its crops' handles expanded);
// the padding rows and the rows of unconstrained jobs: set 0, so the table exists whoever made no set
static void upload_sets(mocr_engine* e, Lane& L) {
    ensure_tok_table(e);
    ensure_set_buffer(e);
    upload_rows(e, L, L.h_sets, (int)MOCR_TOKEN_SET_ALL, e->set_of_row, whole(&Job::sets));
}

// Token automata: the global start state of every row's automaton (a beam batch: by row c K + k, like the sets); the padding
// rows and the rows without an automaton: -1
static void upload_start_states(mocr_engine* e, Lane& L) {
    upload_rows(e, L, L.h_aut, -1, e->aut_base_of_row, [e](const Job& j, int* dst) {
        for (size_t i = 0; i < j.automata.size(); ++i)
            if (j.automata[i] != MOCR_AUTOMATON_NONE) dst[i] = e->aut_first[j.automata[i]];
    });
}

// The decode rows' source of a batch with shared encodings, for the bound lane: allocated by the first batch in which a job
// shares, like the alternatives buffers.
static void ensure_share_buffer(mocr_engine* e) {
    if (!e->src_of_row) e->src_of_row = e->dalloc<int>((size_t)e->Bp);
}

// The three lazily allocated groups of beam buffers, each as the list of its arrays - arr(pointer, elements) for every one, on
// the bound lane's pointers: ensure_beam_*_buffers allocates from the list (Dalloc), mocr_beam_*_state_bytes adds it up (a
// lane's bytes are the same for every lane), so the report cannot drift from the allocation.
struct Dalloc {
    mocr_engine* e;
    template <typename X> void operator()(X*& p, size_t count) const { p = e->dalloc<X>(count); }
};
// what the lanes that hold a group (`has`: the array its ensure function looks at) spend on it
template <typename Has, typename Group> static int64_t beam_group_bytes(mocr_engine* e, Has has, Group group) {
    if (!e) return -1;
    std::lock_guard<std::mutex> lk(e->mu);
    int64_t lanes = 0, bytes = 0;
    for (const Lane& L : e->lanes) lanes += has(L.ctx) ? 1 : 0;
    group(e, [&bytes](auto* p, size_t count) { bytes += (int64_t)(count * sizeof(*p)); });
    return lanes * bytes;
}
// five [Bp] arrays and hyp_ids [Bp][max_len]
static const auto beam_state_arrays = [](mocr_engine* e, auto&& arr) {
    const size_t Bp = (size_t)e->Bp;
    arr(e->beam_score, Bp); arr(e->hyp_score, Bp);
    arr(e->beam_parent, Bp); arr(e->hyp_len, Bp); arr(e->heuristic_open, Bp);
    arr(e->hyp_ids, Bp * e->cfg.max_len);
};
// beam_logp and hyp_logp [Bp][max_len]
static const auto beam_token_arrays = [](mocr_engine* e, auto&& arr) {
    arr(e->beam_logp, (size_t)e->Bp * e->cfg.max_len); arr(e->hyp_logp, (size_t)e->Bp * e->cfg.max_len);
};
// beam_trail and hyp_trail [Bp][max_len], a byte each
static const auto beam_position_arrays = [](mocr_engine* e, auto&& arr) {
    arr(e->beam_trail, (size_t)e->Bp * e->cfg.max_len); arr(e->hyp_trail, (size_t)e->Bp * e->cfg.max_len);
};

// The beam state of the bound lane: allocated by the first beam batch, like the alternatives buffers.
static void ensure_beam_buffers(mocr_engine* e) {
    if (!e->hyp_ids) beam_state_arrays(e, Dalloc{e});
}

// The token form's two histories, for the bound lane: allocated by the first beam batch that asks for token scores or
// brings a token set, so engines that run plain beam batches keep the footprint mocr_beam_state_bytes reports.
static void ensure_beam_token_buffers(mocr_engine* e) {
    if (!e->hyp_logp) beam_token_arrays(e, Dalloc{e});
}

// The automaton form's hypothesis states, for the bound lane (the beams' states and the crops' start states are the greedy
// automaton buffers): allocated by the first beam batch that brings a token automaton.
static void ensure_beam_automaton_buffers(mocr_engine* e) {
    ensure_automaton_buffers(e);
    if (e->hyp_state) return;
    e->hyp_state = e->dalloc<int>((size_t)e->Bp);
}

// The trail form's two histories, for the bound lane: allocated by the first beam batch that asks for token positions.
static void ensure_beam_position_buffers(mocr_engine* e) {
    if (!e->hyp_trail) beam_position_arrays(e, Dalloc{e});
}

// out[r] = in[d_src_of_row[r]] for r < rows, rows of S x D elements of the engine's dtype; `in` holds n_src of them and is
// not `out` (kernels_share.h).
static void launch_enc_expand(mocr_engine* e, const void* in, void* out, const int* d_src_of_row, int n_src, int rows) {
    const size_t row_bytes = (size_t)e->S * e->D * e->esz;
    if (row_bytes % 16 || in == out) throw ArgError{"enc_expand: rows of whole 16-byte pieces, out of place", MOCR_ERR_UNSUPPORTED};
    const int chunks = (int)(row_bytes / 16), per_row = (chunks + EXPAND_THREADS - 1) / EXPAND_THREADS;
    ProfScope ps(e, "enc_expand", 0, 2.0 * rows * (double)row_bytes);
    hipLaunchKernelGGL(enc_expand_kernel, dim3((unsigned)rows * (unsigned)per_row), dim3(EXPAND_THREADS), 0, e->stream,
                       reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out), d_src_of_row, n_src, rows, chunks, per_row);
    HIPCHECK(hipGetLastError());
}

// start_batch, part 1: the jobs' planes staged in d_in, one per distinct source of every job - the encoder runs on n_enc <= n crops
static void stage_planes(mocr_engine* e, const Lane& L) {
    const int IMG = e->cfg.image_size;
    const size_t plane = (size_t)IMG * IMG;
    int plane0 = 0;
    for (const Job& j : L.jobs) {
        uint8_t* gdst = e->d_in + (size_t)plane0 * plane;
        const size_t rowb = (size_t)IMG * j.channels;
        uint8_t* dst = (!j.src_host || j.channels == 1) ? gdst : e->d_rgb + (size_t)plane0 * plane * 3;
        if (j.wait_ev) HIPCHECK(hipStreamWaitEvent(e->stream, j.wait_ev, 0));
        // `count` consecutive planes of the job's source, from plane `first` of it, to the job's plane `at`
        auto copy_planes = [&](int at, int first, int count) {
            if (!j.src_host) {
                HIPCHECK(hipMemcpyAsync(gdst + (size_t)at * plane, j.src + (size_t)first * plane, plane * count, hipMemcpyDeviceToDevice, e->stream));
            } else if (j.row_stride == (int64_t)rowb && j.image_stride == (int64_t)(rowb * IMG)) {
                HIPCHECK(hipMemcpyAsync(dst + (size_t)at * rowb * IMG, j.src + (size_t)first * j.image_stride, rowb * IMG * count,
                                        hipMemcpyHostToDevice, e->stream));
            } else {
                for (int i = 0; i < count; ++i)
                    HIPCHECK(hipMemcpy2DAsync(dst + (size_t)(at + i) * IMG * rowb, rowb, j.src + (size_t)(first + i) * j.image_stride,
                                              j.row_stride, rowb, IMG, hipMemcpyHostToDevice, e->stream));
            }
        };
        if (j.planes.empty()) copy_planes(0, 0, j.n_src);
        else
            for (int i0 = 0, i1; i0 < j.n_src; i0 = i1) {      // runs of neighbouring planes move as one copy
                for (i1 = i0 + 1; i1 < j.n_src && j.planes[i1] == j.planes[i1 - 1] + 1; ++i1) {}
                copy_planes(i0, j.planes[i0], i1 - i0);
            }
        if (j.src_host && j.channels == 3) {
            const long long npix = (long long)j.n_src * IMG * IMG;
            hipLaunchKernelGGL(rgb_to_l_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, e->stream, dst, gdst, npix);
            HIPCHECK(hipGetLastError());
        }
        plane0 += j.n_src;
    }
}

// start_batch, part 2: the staged planes encoded into ENC, one encoding per decode row, and what the attention path reads of them
template <typename T>
static void encode_batch(mocr_engine* e, Lane& L) {
    e->n_encoded += L.n_enc;
    const bool shares = std::any_of(L.jobs.begin(), L.jobs.end(), [](const Job& j) { return !j.src_of_row.empty(); });
    if (!shares) run_encoder<T>(e, e->d_in, L.n);
    else {
        // Shared encodings: the final LayerNorm leaves the n_enc encodings in CTX - dead since the last layer's O-projection -
        // and one gather gives every decode row its own copy in ENC; everything behind it goes by row as always.
        if (L.n_enc > L.n || (size_t)L.n_enc * e->S * e->D * sizeof(T) > e->ctx_cap)
            throw ArgError{"shared encodings: the staging buffer is too small for this batch", MOCR_ERR_STATE};
        ensure_share_buffer(e);
        // (a row's source counts from the job's first plane of the batch, p0; a job that shares nothing: row i reads its plane i)
        upload_rows(e, L, L.h_src, 0, e->src_of_row, [p0 = 0](const Job& j, int* dst) mutable {
            for (int i = 0; i < j.n; ++i) dst[i] = p0 + (j.src_of_row.empty() ? i : j.src_of_row[i]);
            p0 += j.n_src;
        });
        run_encoder<T>(e, e->d_in, L.n_enc, e->CTX);
        launch_enc_expand(e, e->CTX, e->ENC, e->src_of_row, L.n_enc, L.n);
    }
    if (!e->use_latent(L.np0)) run_cross_kv<T>(e, L.n);
    else if (e->fp8attn) quantize_enc(e, L.n);
}

// start_batch, part 3: the decode state of the batch's mode - one block per feature, in stream order the uploads, memsets and
// init kernels of the features, the start token's kernel, the beam state
template <typename T>
static void prepare_decode(mocr_engine* e, Lane& L) {
    const DecMode& m = L.mode;
    // rows read pad_id (= 0) beyond what the loop writes
    HIPCHECK(hipMemsetAsync(e->ids, 0, (size_t)L.np * e->cfg.max_len * sizeof(int), e->stream));
    // Scores: the start token and the pad tail score 0; alternatives: positions the steps do not write read -1 / 0
    if (m.level >= 1) HIPCHECK(hipMemsetAsync(e->scores, 0, (size_t)L.np * e->cfg.max_len * sizeof(float), e->stream));
    if (m.level >= 2) {
        ensure_alt_buffers(e);
        HIPCHECK(hipMemsetAsync(e->alt_ids, 0xFF, (size_t)L.np * e->cfg.max_len * MOCR_ALTERNATIVES * sizeof(int), e->stream));
        HIPCHECK(hipMemsetAsync(e->alt_logp, 0, (size_t)L.np * e->cfg.max_len * MOCR_ALTERNATIVES * sizeof(float), e->stream));
    }
    // token constraints: the merged rows' sets go up before the first decode graph (a prefixed batch runs masked even when
    // nobody made a set: every row reads set 0)
    if (m.mask) upload_sets(e, L);
    // forced prefixes: the merged rows' lengths and tokens (the padding rows and the rows of jobs without a prefix: length 0)
    if (m.prefix) {
        ensure_prefix_buffers(e);
        upload_rows(e, L, L.h_plen, 0, e->prefix_len, whole(&Job::prefix_len));
        const size_t ML = (size_t)e->cfg.max_len;       // a job's [n][prefix_ld] rows, packed, become [np][max_len] ones
        upload_rows(e, L, L.h_prefix, 0, e->prefix, [ML](const Job& j, int* dst) {
            for (size_t i = 0; i < j.prefix_len.size(); ++i) std::copy_n(j.prefix.begin() + i * j.prefix_ld, j.prefix_len[i], dst + i * ML);
        }, ML);
    }
    // no-repeat n-grams: the per-row masks start as the rows' sets (m.ngram implies m.mask: the table and the sets are up)
    if (m.ngram) {
        ensure_ngram_buffers(e);
        upload_rows(e, L, L.h_ngram, 0, e->ngram_of_row, whole(&Job::ngram));
        if (!m.automaton) launch_ngram_init(e, e->row_mask, e->tok_table, e->set_of_row, e->ngram_of_row, L.np);
    }
    // token automata: the rows' start states (the padding rows and the rows without an automaton: -1), their first masks
    if (m.automaton) {
        if (e->V != 6144) throw ArgError{"token automata need the 6144-token vocabulary", MOCR_ERR_UNSUPPORTED};
        if (m.penalty) {
            // (the PEN forms are SOFT forms, and a captured decode graph holds the arena's addresses: the arena and its soft part
            // exist from the first penalty batch on, whether or not a row of it brings an automaton - a row under a hard automaton
            // reads weight 0 / default -1 there)
            ensure_automaton_arena(e);
            ensure_soft_arena(e);
        }
        ensure_automaton_buffers(e);
        upload_start_states(e, L);
        launch_automaton_init(e, e->row_mask, e->tok_table, e->set_of_row, e->ngram_of_row, L.np, e->aut_edge_begin, e->aut_edge_token,
                              e->aut_accepting, e->aut_base_of_row, e->aut_state, m.soft ? e->aut_default_next : nullptr);
    }
    // repetition penalty: the rows' penalties (the padding rows and the rows of jobs without one: 1) and their first seen
    // words, the start token alone
    if (m.penalty) {
        ensure_penalty_buffers(e);
        upload_rows(e, L, L.h_penalty, 1.f, e->penalty_of_row, whole(&Job::penalty));
        launch_penalty_init(e, e->seen_mask, L.np);
    }
    // token positions: position 0, the pad tail and the rows of the jobs that did not ask read 0
    if (m.positions) {
        ensure_pos_buffers(e);
        HIPCHECK(hipMemsetAsync(e->pos_out, 0, (size_t)L.n * e->cfg.max_len * MOCR_POSITION_FIELDS * sizeof(float), e->stream));
    }
    // The decode steps run on np >= n rows (graph_rows): the padding rows are born finished, emit pad_id and read
    // whatever the workspace holds for them (finite values; no kernel mixes rows).
    DecState st = make_state(e, L.max_len, nullptr, 0, nullptr, L.n);
    dec_token<T, true>(e, st, m, 0, L.np);
    // beam search: the start token's kernel is the greedy one; the beam state starts as [0, -1e9, ...] and an empty finished set
    if (m.beam) {
        ensure_beam_buffers(e);
        if (m.beam_tokens) {
            ensure_beam_token_buffers(e);
            upload_sets(e, L);
        }
        if (m.positions) ensure_beam_position_buffers(e);
        if (m.beam_automaton) {     // the crops' start states by row (c K + k, like the sets), padding rows without one
            ensure_beam_automaton_buffers(e);
            upload_start_states(e, L);
            ProfScope pa(e, "beam_automaton_init", 0, (double)L.np * 12);
            hipLaunchKernelGGL(beam_automaton_init_kernel, dim3((L.np + 255) / 256), dim3(256), 0, e->stream, (const int*)e->aut_base_of_row,
                               e->aut_state, e->hyp_state, L.np);
            HIPCHECK(hipGetLastError());
        }
        ProfScope ps(e, "beam_init", 0, (double)L.np * e->cfg.max_len * 4);
        hipLaunchKernelGGL(beam_init_kernel, dim3(L.np), dim3(64), 0, e->stream, make_beam_state(e, m.beam_cfg, m.beam_tokens, m.positions),
                           m.beam_cfg.num_beams, L.np, e->cfg.max_len, e->cfg.pad_id);
        HIPCHECK(hipGetLastError());
    }
}

// The batch runs in the richest mode any of its jobs asked for (mode_of; soft token automata: if any row's automaton is soft)
template <typename T>
void start_batch(mocr_engine* e, Lane& L) {
    L.mode = mode_of(L.jobs);
    if (L.mode.automaton || L.mode.beam_automaton)
        for (const Job& j : L.jobs)
            for (int32_t h : j.automata) L.mode.soft = L.mode.soft || e->aut_soft[h] != 0;
    stage_planes(e, L);
    encode_batch<T>(e, L);
    prepare_decode<T>(e, L);
    L.t = 0; L.steps = L.max_len - 1; L.chunk = 0;
    L.finishing = false;
    L.flag_pending[0] = L.flag_pending[1] = false;
}

// The last two outputs of a job, greedy or beam, from row0 of the batch: its token positions and its rows' (hypotheses') final
// states.  A batch in which nobody brings an automaton keeps no states: every row MOCR_STATE_NONE = -1, a host fill or a device
// memset.
static void copy_out_pos_state(mocr_engine* e, const Lane& L, const Job& j, int row0) {
    const hipMemcpyKind kind = j.out_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (j.out_pos) {
        const size_t ld = (size_t)e->cfg.max_len * MOCR_POSITION_FIELDS;
        HIPCHECK(hipMemcpyAsync(j.out_pos, e->pos_out + row0 * ld, j.n * ld * sizeof(float), kind, e->stream));
    }
    if (j.out_state) {
        if (L.mode.automaton || L.mode.beam_automaton) HIPCHECK(hipMemcpyAsync(j.out_state, e->aut_state_out + row0, (size_t)j.n * sizeof(int), kind, e->stream));
        else if (j.out_host) std::fill(j.out_state, j.out_state + j.n, (int32_t)MOCR_STATE_NONE);
        else HIPCHECK(hipMemsetAsync(j.out_state, 0xFF, (size_t)j.n * sizeof(int), e->stream));
    }
}

void finish_batch(mocr_engine* e, Lane& L) {
    if (L.mode.positions) {      // token positions: the deferred pass over the rows the steps recorded, before the outputs leave
        if (e->cfg.dtype == MOCR_BF16) run_positions<bf16_t>(e, L); else run_positions<float>(e, L);
    }
    const bool beam = L.mode.beam;
    // token automata: the rows' states in their automata's own numbering - a beam batch: the hypotheses' (an empty slot and a crop
    // without an automaton: MOCR_STATE_NONE)
    if (L.mode.automaton || L.mode.beam_automaton) {
        hipLaunchKernelGGL(automaton_state_out_kernel, dim3((L.n + 255) / 256), dim3(256), 0, e->stream,
                           (const int*)(L.mode.beam_automaton ? e->hyp_state : e->aut_state), (const int*)e->aut_base_of_row, e->aut_state_out, L.n);
        HIPCHECK(hipGetLastError());
    }
    // where a job's rows are read from: the rows themselves, or - beam search - the crops' finished sets, [crops][K] = the job's rows
    // (logp: a beam batch with a job that asks ran the token form; positions: it kept the trails and ran the deferred pass over them)
    struct OutView { const int *ids, *len; const float* logp; };
    const OutView from = beam ? OutView{e->hyp_ids, e->hyp_len, e->hyp_logp} : OutView{e->ids, e->len, e->scores};
    const size_t ML = (size_t)e->cfg.max_len;
    size_t row0 = 0;
    for (const Job& j : L.jobs) {
        const hipMemcpyKind kind = j.out_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        HIPCHECK(hipMemcpyAsync(j.out_ids, from.ids + row0 * ML, j.n * ML * sizeof(int), kind, e->stream));
        HIPCHECK(hipMemcpyAsync(j.out_len, from.len + row0, (size_t)j.n * sizeof(int), kind, e->stream));
        if (beam) HIPCHECK(hipMemcpyAsync(j.out_score, e->hyp_score + row0, (size_t)j.n * sizeof(float), kind, e->stream));
        if (j.out_logp) HIPCHECK(hipMemcpyAsync(j.out_logp, from.logp + row0 * ML, j.n * ML * sizeof(float), kind, e->stream));
        if (!beam && j.out_alt_ids) {
            const size_t ld = ML * MOCR_ALTERNATIVES;
            HIPCHECK(hipMemcpyAsync(j.out_alt_ids, e->alt_ids + row0 * ld, j.n * ld * sizeof(int), kind, e->stream));
            HIPCHECK(hipMemcpyAsync(j.out_alt_logp, e->alt_logp + row0 * ld, j.n * ld * sizeof(float), kind, e->stream));
        }
        copy_out_pos_state(e, L, j, (int)row0);
        row0 += j.n;
    }
    L.jobs.clear();
    L.active = false;
}

// Finished rows stop costing (r04).  `unfinished` is the lane's unfinished-row count as of two chunks ago (the early-exit
// flag): rows only ever finish, so at most that many are unfinished now.  When the decode steps could run on a smaller
// graph-friendly row count, the unfinished rows are moved to the first slots (kernels_decode.h: compact_plan_kernel /
// compact_move_kernel, three small launches between two graph replays) and the next chunks run on that many slots.  The
// batch keeps its kernel regime (mocr_engine::regime = the row count it started with): the attention paths keep different
// caches, and with the GEMM tiles and split-K slabs unchanged a row's ids are bit-identical to an uncompacted run's.
// Worth it from a 1/8 cut: every distinct row count is a decode graph of its own.
template <typename T>
void compact_rows(mocr_engine* e, Lane& L, int unfinished) {
    if (e->cfg.flags & MOCR_FLAG_NO_COMPACTION) return;
    // (batches of the one-launch-per-projection path - <= 32 rows - stay as they are: their steps are launch-bound)
    if (!L.mode.beam && e->use_smallm(L.np0)) return;
    const int want = graph_rows(std::max(unfinished, 1), e->cfg.max_batch);
    if (want >= L.np || (long long)want * 8 > (long long)L.np * 7) return;
    ProfScope ps(e, "compact_rows", 0, (double)want * e->D * (4 + sizeof(T)) * 4);
    int* const new_map = e->rowmap_tmp;
    int* const src_slot = e->rowmap_tmp + e->Bp;
    hipLaunchKernelGGL(compact_plan_kernel, dim3(1), dim3(1024), 0, e->stream, (const int*)e->rowmap, (const int*)e->finished, L.np,
                       new_map, src_slot);
    for (int phase = 0; phase < 2; ++phase)
        hipLaunchKernelGGL((compact_move_kernel<T, 768>), dim3(want), dim3(192), 0, e->stream, phase, (const int*)new_map,
                           (const int*)src_slot, e->x_f32, reinterpret_cast<T*>(e->x_t), e->a_f32, reinterpret_cast<T*>(e->a_t), e->rowmap,
                           want, L.np);
    HIPCHECK(hipGetLastError());
    L.np = want;
    e->n_compactions += 1;
}

// Enqueue the next chunk of lane L (or finish it).  Blocks only on a flag two chunks old.
template <typename T>
void advance(mocr_engine* e, Lane& L) {
    const bool early = !(e->cfg.flags & MOCR_FLAG_NO_EARLY_EXIT);
    const int slot = L.chunk & 1;
    if (early) {
        // The unfinished-row count this chunk is planned with: the flag of the chunk just before it when that has already
        // landed (it has whenever another lane's work ran in between - no wait), otherwise the flag two chunks back, waited
        // for as always (the lane then still has a chunk queued while the host looks).  A fresher count compacts a batch -
        // and ends it - up to a chunk earlier; when the rows move does not change any id (compact_rows).
        int unf = -1;
        const int newer = slot ^ 1;
        if (L.flag_pending[newer]) {
            const hipError_t q = hipEventQuery(L.flag_ev[newer]);
            if (q == hipSuccess) {
                unf = e->h_pinned[newer];
                L.flag_pending[newer] = L.flag_pending[slot] = false;      // (the older flag's event precedes it in the stream)
            } else {
                (void)hipGetLastError();                                   // hipErrorNotReady is not a failure
                if (q != hipErrorNotReady) HIPCHECK(q);
            }
        }
        if (unf < 0 && L.flag_pending[slot]) {
            HIPCHECK(hipEventSynchronize(L.flag_ev[slot]));
            L.flag_pending[slot] = false;
            unf = e->h_pinned[slot];
        }
        if (unf >= 0) {
            if (unf <= 0) { finish_batch(e, L); return; }
            if (unf < L.n) L.finishing = true;
            if (e->D == 768) compact_rows<T>(e, L, unf);
        }
    }
    if (L.t >= L.steps) { finish_batch(e, L); return; }
    DecState st = make_state(e, L.max_len, nullptr, 0, nullptr, L.n, L.mode);
    // (while rows are leaving, half-length chunks: the count a compaction acts on is at most 4 + 4 steps old instead of 8 + 8;
    // a batch none of whose rows has finished - the synthetic-weights headline - keeps the long chunks)
    const int chunk = L.finishing ? std::min(chunk_steps(L.np), CHUNK / 2) : chunk_steps(L.np);
    const int k = std::min(chunk, L.steps - L.t);
    const bool use_graph = !e->prof_on && !(e->cfg.flags & MOCR_FLAG_NO_GRAPH);
    if (use_graph && k == chunk) {
        HIPCHECK(hipGraphLaunch(decode_graph<T>(e, st, L.mode, L.np, chunk, L.t), e->stream));
    } else {
        for (int i = 0; i < k; ++i) {
            if (use_graph) HIPCHECK(hipGraphLaunch(decode_graph<T>(e, st, L.mode, L.np, 1, L.t + i), e->stream));
            else decode_step<T>(e, st, L.mode, L.np, L.t + i);
        }
    }
    L.t += k;
    e->n_slot_steps += (long long)L.np * k;
    if (early) {
        HIPCHECK(hipMemcpyAsync(e->h_pinned + slot, e->n_unf, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipEventRecord(L.flag_ev[slot], e->stream));
        L.flag_pending[slot] = true;
    }
    L.chunk += 1;
}

// One scheduling pass over the lanes: an idle lane takes as many pending requests as fit in
// max_batch rows (FIFO, same max_len) and runs them as ONE batch; busy lanes get one chunk.
template <typename T>
bool pump_once(mocr_engine* e) {
    bool any = false;
    for (size_t i = 0; i < e->lanes.size(); ++i) {
        Lane& L = e->lanes[i];
        if (!L.active && !e->pending.empty()) {
            L.jobs.clear();
            L.n = L.n_enc = 0;
            L.max_len = e->pending.front().max_len;
            // An idle lane takes as many queued requests as fit in max_batch rows.  When SEVERAL lanes are idle and the
            // queue would fit into fewer of them, it is split evenly over the idle lanes as long as every part keeps
            // >= SPLIT_MIN rows: two fat batches in flight overlap each other's latency-bound phases (+6 % at 2 x 2560
            // against 1 x 5120 rows, r02), while below that merging beats overlapping.
            // (r03: 600 instead of 1024 - the 1250 rows a rank of the 8-GPU queue run gets decoded as 2 x 625 in 258 ms
            // instead of 270 ms as one batch.  r04, with three attention blocks per CU and the fused query kernel from 512
            // rows, tools/r04_probe_lanes.sh: 1250 rows as ONE batch 216-221 ms against 229-231 ms as 2 x 625; 2500 rows 370-378
            // as one against 374-381 as 2 x 1250 (3 x 833: 390); 2 x 2560 against 1 x 5120: +5.5 %.  Parts below ~1280 rows lose.)
            static const long long SPLIT_MIN = env_int("MOCR_SPLIT_MIN", 1280);
            long long rows_pending = 0;
            for (const Job& p : e->pending) rows_pending += p.n;
            int idle = 0;
            for (size_t k = i; k < e->lanes.size(); ++k) idle += e->lanes[k].active ? 0 : 1;
            long long cap = e->cfg.max_batch;
            if (idle > 1 && !e->prof_on && rows_pending < (long long)idle * cap) {     // (instrumented passes: one batch, no overlap)
                const int parts = (int)std::max<long long>(1, std::min<long long>(idle, rows_pending / SPLIT_MIN));
                cap = std::min<long long>(cap, (rows_pending + parts - 1) / parts);
            }
            size_t take = 0;
            // (beam search: a batch is all beam jobs of one configuration, or has none)
            const mocr_beam_config front_beam = e->pending.front().beam;
            while (take < e->pending.size() && e->pending[take].max_len == L.max_len && same_beam(e->pending[take].beam, front_beam) &&
                   (take == 0 || L.n + e->pending[take].n <= cap) && L.n + e->pending[take].n <= e->cfg.max_batch) {
                L.n += e->pending[take].n;
                L.n_enc += e->pending[take].n_src;
                L.jobs.push_back(e->pending[take]);
                ++take;
            }
            e->pending.erase(e->pending.begin(), e->pending.begin() + take);
            L.np = L.np0 = graph_rows(L.n, e->cfg.max_batch);
            L.active = true;
            e->bind((int)i);
            { RegimeScope rs(e, L.np0); start_batch<T>(e, L); }
            e->unbind((int)i);
        }
        if (L.active) {
            e->bind((int)i);
            { RegimeScope rs(e, L.np0); advance<T>(e, L); }
            e->unbind((int)i);
            any = true;
        }
    }
    return any || !e->pending.empty();
}

// Run every submitted job to completion and wait for the GPU.
void drive(mocr_engine* e) {
    try {
        if (e->cfg.dtype == MOCR_BF16) { while (pump_once<bf16_t>(e)) {} }
        else { while (pump_once<float>(e)) {} }
    } catch (...) {      // (the batch's mode lives in its lane and its regime in a RegimeScope: nothing of either to restore here)
        e->pending.clear();
        for (auto& L : e->lanes) { L.active = false; L.jobs.clear(); (void)hipStreamSynchronize(L.ctx.stream); }
        throw;
    }
    for (auto& L : e->lanes) HIPCHECK(hipStreamSynchronize(L.ctx.stream));
}

void submit(mocr_engine* e, const Job& j) {
    e->pending.push_back(j);
    long long rows = 0;
    for (const Job& p : e->pending) rows += p.n;
    if (rows >= e->cfg.max_batch) {   // a full batch is waiting: get the GPU going; else wait for more to merge
        if (e->cfg.dtype == MOCR_BF16) pump_once<bf16_t>(e); else pump_once<float>(e);
    }
}

// ---------------------------------------------------------------------------------------- weights
struct Uploader {
    mocr_engine* e;
    const std::vector<float>& get(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = e->host_w.find(name);
        if (it == e->host_w.end()) throw ArgError{"missing tensor " + name, MOCR_ERR_STATE};
        const auto& shp = e->host_shape[name];
        std::vector<int64_t> want(shape);
        if (shp != want) throw ArgError{"bad shape for tensor " + name, MOCR_ERR_ARG};
        return it->second;
    }
    float* f32(const std::vector<float>& v) {
        float* d = e->dalloc<float>(v.size());
        HIPCHECK(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return d;
    }
    void* mat(const std::vector<float>& v) {  // GEMM operand in the engine dtype
        if (e->cfg.dtype == MOCR_F32) return f32(v);
        std::vector<uint16_t> h(v.size());
        for (size_t i = 0; i < v.size(); ++i) h[i] = host_f2bf(v[i]);
        uint16_t* d = e->dalloc<uint16_t>(h.size());
        HIPCHECK(hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        return d;
    }
};

static std::vector<float> concat(std::initializer_list<const std::vector<float>*> parts) {
    std::vector<float> out;
    for (auto* p : parts) out.insert(out.end(), p->begin(), p->end());
    return out;
}

// Is this checkpoint's residual stream one the LayerNorm fold may round to bf16?  Eight probe crops (six of seeded noise, one
// white, one black) go through the encoder with the LayerNorms as launches; in front of each of the 24 foldable LayerNorms
// the stream is copied out and the rounding-noise ratio of calib_observe is taken.  Synthetic N(0, 0.02^2) weights: ~1.0-1.1.
// A stream with a DC offset of several sigma (trained ViTs): several - the fold would cost that factor in GEMM input noise,
// and stays off.  Run once per engine, at commit (~30 ms); mocr_ln_fold_state reports the outcome.
constexpr double FOLD_RATIO_MAX = 1.5;
void calibrate_ln_fold(mocr_engine* e, mocr_engine::FoldCalib& cal) {
    const int n = 8;
    if (e->cfg.max_batch < 56 || e->D != 768 || e->lanes.empty()) return;      // batches this small never take the persistent GEMMs
    const size_t plane = (size_t)e->cfg.image_size * e->cfg.image_size;
    std::vector<uint8_t> probe(n * plane);
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < 6 * plane; ++i) { lcg = lcg * 1664525u + 1013904223u; probe[i] = (uint8_t)(lcg >> 24); }
    std::fill(probe.begin() + 6 * plane, probe.begin() + 7 * plane, (uint8_t)255);
    std::fill(probe.begin() + 7 * plane, probe.end(), (uint8_t)0);
    e->bind(0);
    HIPCHECK(hipMemcpyAsync(e->d_in, probe.data(), probe.size(), hipMemcpyHostToDevice, e->stream));
    cal.idx = 0; cal.worst = 0.0;
    e->calib = &cal;
    try {
        run_encoder<bf16_t>(e, e->d_in, n);
        HIPCHECK(hipStreamSynchronize(e->stream));
    } catch (...) {
        e->calib = nullptr;
        e->unbind(0);
        throw;
    }
    e->calib = nullptr;
    e->unbind(0);
    e->fold_ratio = (float)cal.worst;
    e->fold_ok = cal.worst <= FOLD_RATIO_MAX;
}

void commit_weights(mocr_engine* e) {
    const auto& c = e->cfg;
    const int64_t D = c.hidden, F = c.ffn, V = c.vocab, P = c.patch_size, S = e->S;
    Uploader up{e};
    mocr_engine::FoldCalib ln_gb;
    auto& w = e->w;
    // pixel LUT, exactly the HF image processor's arithmetic (float64 rescale, float32 normalise)
    {
        std::vector<float> lut(256);
        for (int u = 0; u < 256; ++u) {
            const float x = (float)((double)u * (1.0 / 255.0));
            lut[u] = (x - 0.5f) / 0.5f;
        }
        w.lut = up.f32(lut);
    }
    // patch embedding: the three input channels are identical, so sum the kernel over channels
    {
        const auto& pw = up.get("encoder.embeddings.patch_embeddings.projection.weight", {D, 3, P, P});
        std::vector<float> ws((size_t)D * P * P);
        for (int64_t o = 0; o < D; ++o)
            for (int64_t k = 0; k < P * P; ++k) {
                double s = 0;
                for (int ch = 0; ch < 3; ++ch) s += pw[(o * 3 + ch) * P * P + k];
                ws[o * P * P + k] = (float)s;
            }
        w.wpe = up.mat(ws);
        w.bpe = up.f32(up.get("encoder.embeddings.patch_embeddings.projection.bias", {D}));
        w.cls = up.f32(up.get("encoder.embeddings.cls_token", {1, 1, D}));
        w.pos_enc = up.f32(up.get("encoder.embeddings.position_embeddings", {1, S, D}));
    }
    w.enc.resize(c.enc_layers);
    for (int l = 0; l < c.enc_layers; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        EncLayerW& L = w.enc[l];
        L.wqkv = up.mat(concat({&up.get(p + "attention.q_proj.weight", {D, D}), &up.get(p + "attention.k_proj.weight", {D, D}),
                                &up.get(p + "attention.v_proj.weight", {D, D})}));
        L.bqkv = up.f32(concat({&up.get(p + "attention.q_proj.bias", {D}), &up.get(p + "attention.k_proj.bias", {D}),
                                &up.get(p + "attention.v_proj.bias", {D})}));
        L.wo = up.mat(up.get(p + "attention.o_proj.weight", {D, D}));
        L.bo = up.f32(up.get(p + "attention.o_proj.bias", {D}));
        L.ln1g = up.f32(up.get(p + "layernorm_before.weight", {D}));
        L.ln1b = up.f32(up.get(p + "layernorm_before.bias", {D}));
        L.ln2g = up.f32(up.get(p + "layernorm_after.weight", {D}));
        L.ln2b = up.f32(up.get(p + "layernorm_after.bias", {D}));
        L.w1 = up.mat(up.get(p + "mlp.fc1.weight", {F, D}));
        L.b1 = up.f32(up.get(p + "mlp.fc1.bias", {F}));
        L.w2 = up.mat(up.get(p + "mlp.fc2.weight", {D, F}));
        L.b2 = up.f32(up.get(p + "mlp.fc2.bias", {D}));
        if (c.dtype == MOCR_BF16) {
            // LN(x) W^T + b = rstd (x (W o gamma)^T - mean colsum) + (b + W beta): the folded operands (colsum of the ROUNDED
            // folded weight - what the MFMAs multiply -, in double)
            auto fold = [&](const std::vector<float>& W, const std::vector<float>& b, const std::vector<float>& g, const std::vector<float>& be,
                            int64_t N, void*& wf, float*& cs, float*& bf) {
                std::vector<float> Wf((size_t)N * D), csum(N), bias(N);
                for (int64_t n = 0; n < N; ++n) {
                    double sc = 0.0, sb = 0.0;
                    for (int64_t k = 0; k < D; ++k) {
                        const float v = W[n * D + k] * g[k];
                        Wf[n * D + k] = v;
                        sc += (double)host_bf2f(host_f2bf(v));
                        sb += (double)W[n * D + k] * (double)be[k];
                    }
                    csum[n] = (float)sc;
                    bias[n] = (float)((double)b[n] + sb);
                }
                wf = up.mat(Wf); cs = up.f32(csum); bf = up.f32(bias);
            };
            const auto wqkv_h = concat({&up.get(p + "attention.q_proj.weight", {D, D}), &up.get(p + "attention.k_proj.weight", {D, D}),
                                        &up.get(p + "attention.v_proj.weight", {D, D})});
            const auto bqkv_h = concat({&up.get(p + "attention.q_proj.bias", {D}), &up.get(p + "attention.k_proj.bias", {D}),
                                        &up.get(p + "attention.v_proj.bias", {D})});
            fold(wqkv_h, bqkv_h, up.get(p + "layernorm_before.weight", {D}), up.get(p + "layernorm_before.bias", {D}), 3 * D,
                 L.wqkv_f, L.sqkv, L.bqkv_f);
            ln_gb.g.push_back(up.get(p + "layernorm_before.weight", {D})); ln_gb.b.push_back(up.get(p + "layernorm_before.bias", {D}));
            ln_gb.g.push_back(up.get(p + "layernorm_after.weight", {D})); ln_gb.b.push_back(up.get(p + "layernorm_after.bias", {D}));
            fold(up.get(p + "mlp.fc1.weight", {F, D}), up.get(p + "mlp.fc1.bias", {F}), up.get(p + "layernorm_after.weight", {D}),
                 up.get(p + "layernorm_after.bias", {D}), F, L.w1_f, L.s1, L.b1_f);
        }
    }
    w.lnfg = up.f32(up.get("encoder.layernorm.weight", {D}));
    w.lnfb = up.f32(up.get("encoder.layernorm.bias", {D}));
    // Static e4m3 scale of a LayerNorm output: |gamma_k z_k + beta_k| <= max|gamma| sqrt(D - 1) + max|beta| for ANY input
    // (a normalised vector's element is at most sqrt(D - 1)), mapped onto e4m3's largest finite value 448.
    auto ln_scale = [&](const std::string& gname, const std::string& bname) {
        float gm = 0.f, bm = 0.f;
        for (float v : up.get(gname, {D})) gm = std::max(gm, std::fabs(v));
        for (float v : up.get(bname, {D})) bm = std::max(bm, std::fabs(v));
        return (gm * std::sqrt((float)(D - 1)) + bm) / 448.0f;
    };
    w.sx_enc = ln_scale("encoder.layernorm.weight", "encoder.layernorm.bias");
    w.sx_self.assign(c.dec_layers, 1.f);
    w.sx_self[0] = ln_scale("decoder.bert.embeddings.LayerNorm.weight", "decoder.bert.embeddings.LayerNorm.bias");
    for (int l = 1; l < c.dec_layers; ++l) {
        const std::string pp = "decoder.bert.encoder.layer." + std::to_string(l - 1) + ".output.LayerNorm.";
        w.sx_self[l] = ln_scale(pp + "weight", pp + "bias");
    }
    const std::string d = "decoder.bert.";
    w.word = up.f32(up.get(d + "embeddings.word_embeddings.weight", {V, D}));
    w.posd = up.f32(up.get(d + "embeddings.position_embeddings.weight", {(int64_t)c.max_pos, D}));
    {
        const auto& tt = e->host_w.at(d + "embeddings.token_type_embeddings.weight");
        std::vector<float> t0(tt.begin(), tt.begin() + D);
        w.type0 = up.f32(t0);
    }
    w.embg = up.f32(up.get(d + "embeddings.LayerNorm.weight", {D}));
    w.embb = up.f32(up.get(d + "embeddings.LayerNorm.bias", {D}));
    w.dec.resize(c.dec_layers);
    std::vector<float> ckv_w, ckv_b;
    for (int l = 0; l < c.dec_layers; ++l) {
        const std::string p = d + "encoder.layer." + std::to_string(l) + ".";
        DecLayerW& L = w.dec[l];
        const std::string a = p + "attention.", x = p + "crossattention.";
        L.wqkv = up.mat(concat({&up.get(a + "self.query.weight", {D, D}), &up.get(a + "self.key.weight", {D, D}),
                                &up.get(a + "self.value.weight", {D, D})}));
        L.bqkv = up.f32(concat({&up.get(a + "self.query.bias", {D}), &up.get(a + "self.key.bias", {D}),
                                &up.get(a + "self.value.bias", {D})}));
        if (e->latent) {
            auto transposed_scaled = [&](const std::vector<float>& wk) {
                std::vector<float> t((size_t)D * D);
                for (int64_t o = 0; o < D; ++o)
                    for (int64_t i = 0; i < D; ++i) t[i * D + o] = wk[o * D + i] * 0.125f;   // [in][out], 1/sqrt(64) folded in
                return t;
            };
            L.wkT_s = up.mat(transposed_scaled(up.get(a + "self.key.weight", {D, D})));
            L.wkT_c = up.mat(transposed_scaled(up.get(x + "self.key.weight", {D, D})));
        }
        L.wo = up.mat(up.get(a + "output.dense.weight", {D, D}));
        L.bo = up.f32(up.get(a + "output.dense.bias", {D}));
        L.ln1g = up.f32(up.get(a + "output.LayerNorm.weight", {D}));
        L.ln1b = up.f32(up.get(a + "output.LayerNorm.bias", {D}));
        L.wqc = up.mat(up.get(x + "self.query.weight", {D, D}));
        L.bqc = up.f32(up.get(x + "self.query.bias", {D}));
        for (const char* kv : {"self.key.", "self.value."}) {
            const auto& ww = up.get(x + kv + "weight", {D, D});
            const auto& bb = up.get(x + kv + "bias", {D});
            ckv_w.insert(ckv_w.end(), ww.begin(), ww.end());
            ckv_b.insert(ckv_b.end(), bb.begin(), bb.end());
        }
        L.woc = up.mat(up.get(x + "output.dense.weight", {D, D}));
        L.boc = up.f32(up.get(x + "output.dense.bias", {D}));
        L.ln2g = up.f32(up.get(x + "output.LayerNorm.weight", {D}));
        L.ln2b = up.f32(up.get(x + "output.LayerNorm.bias", {D}));
        L.w1 = up.mat(up.get(p + "intermediate.dense.weight", {F, D}));
        L.b1 = up.f32(up.get(p + "intermediate.dense.bias", {F}));
        L.w2 = up.mat(up.get(p + "output.dense.weight", {D, F}));
        L.b2 = up.f32(up.get(p + "output.dense.bias", {D}));
        L.ln3g = up.f32(up.get(p + "output.LayerNorm.weight", {D}));
        L.ln3b = up.f32(up.get(p + "output.LayerNorm.bias", {D}));
    }
    w.wckv = up.mat(ckv_w);
    w.bckv = up.f32(ckv_b);
    w.zero_bias = up.f32(std::vector<float>((size_t)D, 0.f));
    const std::string cl = "decoder.cls.predictions.";
    w.wt = up.mat(up.get(cl + "transform.dense.weight", {D, D}));
    w.bt = up.f32(up.get(cl + "transform.dense.bias", {D}));
    w.lntg = up.f32(up.get(cl + "transform.LayerNorm.weight", {D}));
    w.lntb = up.f32(up.get(cl + "transform.LayerNorm.bias", {D}));
    w.wv = up.mat(up.get(cl + "decoder.weight", {V, D}));
    w.bv = up.f32(up.get(cl + "decoder.bias", {V}));
    if (c.dtype == MOCR_BF16) init_kernel_attrs<bf16_t>(); else init_kernel_attrs<float>();
    e->host_w.clear();
    e->host_shape.clear();
    e->committed = true;
    if (c.dtype == MOCR_BF16 && !ln_gb.g.empty()) calibrate_ln_fold(e, ln_gb);
}

void compute_geometry(mocr_engine* e) {
    const auto& c = e->cfg;
    e->S = (c.image_size / c.patch_size) * (c.image_size / c.patch_size) + 1;
    e->G = c.image_size / c.patch_size;
    e->D = c.hidden; e->H = c.heads; e->F = c.ffn; e->V = c.vocab;
    e->esz = c.dtype == MOCR_BF16 ? 2 : 4;
    e->Bp = round_up(c.max_batch, 128);
    e->Mp = round_up(c.max_batch * e->S, 256) + 256;
    e->NCKV = c.dec_layers * 2 * c.hidden;
}

// Workspace of ONE lane, allocated into the engine's bound LaneCtx (then saved with unbind()).
void allocate_lane(mocr_engine* e, int lane_id) {
    const auto& c = e->cfg;
    static_cast<LaneCtx&>(*e) = LaneCtx{};
    e->lane_id = lane_id;
    HIPCHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    const size_t Mp = e->Mp, D = e->D, Bp = e->Bp, esz = e->esz;
    e->d_in = e->dalloc<uint8_t>((size_t)c.max_batch * c.image_size * c.image_size);
    e->d_rgb = e->dalloc<uint8_t>((size_t)c.max_batch * c.image_size * c.image_size * 3);
    e->X = e->dalloc<float>(Mp * D);
    e->Xn = e->dalloc<char>(Mp * D * esz);
    if (c.dtype == MOCR_BF16) {
        e->ln_part = e->dalloc<float>(Mp * 8);
        HIPCHECK(hipMemset(e->ln_part, 0, Mp * 8 * sizeof(float)));      // (partial 3 stays zero: N = 768 has three column slices)
    }
    e->QKV = e->dalloc<char>(Mp * 3 * D * esz);
    e->ctx_cap = Mp * D * esz;      // (also the staging buffer of shared encodings: start_batch checks a batch against it)
    e->CTX = e->dalloc<char>(e->ctx_cap);
    e->Hb = e->dalloc<char>(Mp * (size_t)e->F * esz);
    e->ENC = e->dalloc<char>(Mp * D * esz);
    if (e->latent && e->classic_rows < c.max_batch) {      // else every batch takes the classic kernels
        e->q_t = e->dalloc<char>(Bp * D * esz);
        e->qt = e->dalloc<char>(Bp * 16 * D * esz);
        e->et = e->dalloc<char>(Bp * 16 * D * esz);
        if (!e->fp8attn) e->xcache = e->dalloc<char>(((size_t)c.dec_layers * Bp * c.max_len + 64) * D * esz);
        else {
            e->x8cache = e->dalloc<uint8_t>(((size_t)c.dec_layers * Bp * c.max_len + 64) * D);
            e->enc8 = e->dalloc<uint8_t>((Mp + 64) * D);
        }
    }
    if (e->Bc > 0) {      // classic K/V: the whole engine (fp32 / MOCR_FLAG_CLASSIC_ATTENTION) or its small batches
        const size_t Mc = (size_t)round_up(e->Bc * e->S, 256) + 256;
        e->CKV = e->dalloc<char>(Mc * (size_t)e->NCKV * esz);
        const size_t cache = (size_t)c.dec_layers * e->Bc * e->H * c.max_len * 64 * esz;
        e->kcache = e->dalloc<char>(cache);
        e->vcache = e->dalloc<char>(cache);
    }
    e->slab_cap = (long long)Bp * 12288;
    e->slabs = e->dalloc<float>((size_t)e->slab_cap);
    e->cand_val = e->dalloc<float>((size_t)Bp * (e->V / 64)); e->cand_idx = e->dalloc<int>((size_t)Bp * (e->V / 64));
    e->cand_sum = e->dalloc<float>((size_t)Bp * (e->V / 64)); e->scores = e->dalloc<float>(Bp * (size_t)c.max_len);
    e->x_f32 = e->dalloc<float>(Bp * D); e->a_f32 = e->dalloc<float>(Bp * D); e->c_f32 = e->dalloc<float>(Bp * D);
    e->ln_stats = e->dalloc<float>(3 * Bp * 2);
    e->x_t = e->dalloc<char>(Bp * D * esz); e->a_t = e->dalloc<char>(Bp * D * esz); e->c_t = e->dalloc<char>(Bp * D * esz);
    e->ctx_t = e->dalloc<char>(Bp * D * esz); e->z_t = e->dalloc<char>(Bp * D * esz);
    e->h_t = e->dalloc<char>(Bp * (size_t)e->F * esz);
    e->ids = e->dalloc<int>(Bp * (size_t)c.max_len);
    e->step = e->dalloc<int>(Bp); e->finished = e->dalloc<int>(Bp); e->len = e->dalloc<int>(Bp); e->n_unf = e->dalloc<int>(4);
    e->rowmap = e->dalloc<int>(Bp); e->rowmap_tmp = e->dalloc<int>(2 * Bp);
    HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_pinned), 64, hipHostMallocDefault));
}

void allocate_lanes(mocr_engine* e) {
    compute_geometry(e);
    e->latent = e->cfg.dtype == MOCR_BF16 && !(e->cfg.flags & MOCR_FLAG_CLASSIC_ATTENTION);
    e->fp8attn = e->latent && (e->cfg.flags & MOCR_FLAG_FP8_ATTENTION);
    e->lat_tk = (e->cfg.flags & MOCR_FLAG_LATENT_TILE32) ? 32 : env_int("MOCR_LAT_TK", 18);
    // Small batches of a latent engine take the classic kernels: the persistent latent kernel walks a sequence's key
    // tiles serially on ONE CU (~20 us per call whatever the batch), the classic one spreads a row over 12 blocks.
    // Measured (r01, 300 tokens): 8 rows 36 vs 73 ms, 64 rows 50 vs 80 ms, 256 rows 111 vs 116 ms; r02, both paths with
    // non-temporal key loads: 320 rows 116 vs 126 ms, 384 rows 119 vs 129 ms, 448 / 512 rows (one graph shape) 159 vs 148 ms;
    // r04, latent on three blocks per CU (tools/r04_classic_rows_ab.sh, isolated batch, classic / latent, ms): 192 rows 76.8 /
    // 90.2, 256 rows 90.3 / 96.1, 320 rows 113.3 / 107.7, 384 rows 116.1 / 110.5 - the switch moved from 384 to 256 rows.
    e->classic_rows = !e->latent ? 0 : (e->cfg.flags & MOCR_FLAG_LATENT_ALWAYS) ? 0 : std::min(env_int("MOCR_CLASSIC_ROWS", 256), e->cfg.max_batch);
    e->Bc = e->latent ? e->classic_rows : e->Bp;
    e->smallm_rows = (e->cfg.dtype == MOCR_BF16 && e->D == 768 && e->F == 3072 && e->V % SM_NT == 0 && !(e->cfg.flags & MOCR_FLAG_NO_SMALL_BATCH_PATH))
                         ? std::min(SM_MAX_ROWS, env_int("MOCR_SMALLM_ROWS", SM_MAX_ROWS)) : 0;
    const int nl = std::max(1, std::min(16, (int)e->cfg.lanes));
    e->lanes.resize(nl);
    for (int i = 0; i < nl; ++i) {
        allocate_lane(e, i);
        e->unbind(i);
        HIPCHECK(hipEventCreateWithFlags(&e->lanes[i].flag_ev[0], hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&e->lanes[i].flag_ev[1], hipEventDisableTiming));
    }
    e->bind(0);
    HIPCHECK(hipStreamCreateWithFlags(&e->prep_stream, hipStreamNonBlocking));
}

static void set_error(mocr_engine* e, const std::string& msg) {
    std::lock_guard<std::mutex> lk(e->err_mu);
    e->err = msg;
}

template <typename F> int guarded(mocr_engine* e, F&& f) {
    if (!e) return MOCR_ERR_ARG;
    if (e->poisoned.load(std::memory_order_acquire)) {
        // after a failed HIP call (a fault, a lost device) the context is not trustworthy and HIP keeps
        // returning the same error: refuse instead of serving from a half-dead engine
        return MOCR_ERR_STATE;
    }
    try {
        f();
        return MOCR_OK;
    } catch (const HipError& h) {
        char buf[512];
        snprintf(buf, sizeof(buf), "HIP error %d (%s) at engine.hip:%d: %s - the engine refuses further calls (MOCR_ERR_STATE) until it is destroyed",
                 (int)h.code, hipGetErrorString(h.code), h.line, h.what);
        set_error(e, buf);
        e->poisoned.store(true, std::memory_order_release);
        return MOCR_ERR_HIP;
    } catch (const ArgError& a) {
        set_error(e, a.msg);
        return a.code;
    } catch (const std::bad_alloc&) {
        set_error(e, "host allocation failed");
        return MOCR_ERR_NOMEM;
    } catch (const std::exception& x) {
        set_error(e, x.what());
        return MOCR_ERR_STATE;
    }
}

// The frame of an operator hook: under the engine's lock and on its device, with every submitted job run to completion, f runs
// on lane 0's buffers and stream, and the stream is waited for.  (A hook that checks arguments BEFORE the jobs are driven keeps
// its own frame: with jobs pending the order shows.)
template <typename F> int op_hook(mocr_engine* e, F&& f) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->bind(0);
        f();
        HIPCHECK(hipStreamSynchronize(e->stream));
    });
}

void require_ready(mocr_engine* e, int n, bool bounded = true) {
    if (!e->committed) throw ArgError{"weights not committed (mocr_commit_weights)", MOCR_ERR_STATE};
    if (n <= 0) throw ArgError{"n must be positive", MOCR_ERR_ARG};
    if (bounded && n > e->cfg.max_batch) throw ArgError{"n exceeds max_batch", MOCR_ERR_ARG};
}

// run fn with T = storage type of the engine: fn(bf16_t{}) or fn(float{})
template <typename Fn> void dispatch(mocr_engine* e, Fn&& fn) {
    if (e->cfg.dtype == MOCR_BF16) fn(bf16_t{}); else fn(float{});
}

}  // namespace

// ============================================================================================ C ABI
extern "C" {

int mocr_abi_version(void) { return MOCR_ABI_VERSION; }

int mocr_create(const mocr_config* cfg, mocr_engine** out) {
    if (!cfg || !out || cfg->struct_size != (int32_t)sizeof(mocr_config)) return MOCR_ERR_ARG;
    if (cfg->hidden != 768 || cfg->heads != 12 || cfg->image_size != 224 || cfg->patch_size != 16 || cfg->ffn % 128 ||
        cfg->vocab != 6144 || cfg->max_len < 2 || cfg->max_len > 320 || cfg->max_len > cfg->max_pos || cfg->max_batch < 1 ||
        (cfg->dtype != MOCR_F32 && cfg->dtype != MOCR_BF16) || cfg->enc_layers < 1 || cfg->dec_layers < 1 ||
        cfg->pad_id != 0 || cfg->lanes < 0)
        return MOCR_ERR_UNSUPPORTED;
    mocr_engine* e = new (std::nothrow) mocr_engine();
    if (!e) return MOCR_ERR_NOMEM;
    e->cfg = *cfg;
    e->gen_max_len = cfg->max_len;
    if (e->cfg.lanes == 0) e->cfg.lanes = 1;
    int rc = guarded(e, [&] {
        int ndev = 0;
        HIPCHECK(hipGetDeviceCount(&ndev));
        if (ndev <= 0) throw ArgError{"no HIP device visible: the Manga-OCR engine needs a GPU", MOCR_ERR_HIP};
        HIPCHECK(hipSetDevice(cfg->device));
        {
            int cus = 0;
            HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device));
            e->num_cus = cus >= 8 ? cus / 8 * 8 : 8;
        }
        allocate_lanes(e);
    });
    if (rc != MOCR_OK) {
        fprintf(stderr, "mocr_create failed: %s\n", mocr_last_error(e));
        mocr_destroy(e);
        return rc;
    }
    *out = e;
    return MOCR_OK;
}

void mocr_destroy(mocr_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    for (auto& L : e->lanes)
        if (L.ctx.stream) (void)hipStreamSynchronize(L.ctx.stream);
    for (auto& r : e->recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    for (auto* sc : {&e->rs_src, &e->rs_tmp, &e->rs_desc, &e->rs_coef, &e->rs_bounds, &e->rs_gray})
        if (sc->p) (void)hipFree(sc->p);
    for (auto& sp : e->rs_pin)
        if (sp.p) (void)hipHostFree(sp.p);
    if (e->prep_stream) (void)hipStreamDestroy(e->prep_stream);
    for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
    for (void* p : e->allocs) (void)hipFree(p);
    for (auto& L : e->lanes) {
        if (L.ctx.h_pinned) (void)hipHostFree(L.ctx.h_pinned);
        for (auto ev : L.flag_ev) if (ev) (void)hipEventDestroy(ev);
        if (L.ctx.stream) (void)hipStreamDestroy(L.ctx.stream);
    }
    delete e;
}

const char* mocr_last_error(const mocr_engine* e) {
    if (!e) return "null engine";
    // a copy taken under the error mutex, owned by the calling thread: valid until that thread's next call of this
    // function, whatever other threads do to the engine meanwhile
    static thread_local std::string copy;
    mocr_engine* m = const_cast<mocr_engine*>(e);
    std::lock_guard<std::mutex> lk(m->err_mu);
    copy = m->err;
    return copy.c_str();
}

int mocr_set_tensor(mocr_engine* e, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    return guarded(e, [&] {
        if (!name || !data || !shape || ndim < 1 || ndim > 4) throw ArgError{"mocr_set_tensor: bad argument", MOCR_ERR_ARG};
        if (e->committed) throw ArgError{"weights already committed", MOCR_ERR_STATE};
        std::lock_guard<std::mutex> lk(e->mu);
        int64_t count = 1;
        for (int i = 0; i < ndim; ++i) count *= shape[i];
        e->host_w[name].assign(data, data + count);
        e->host_shape[name].assign(shape, shape + ndim);
    });
}

int mocr_commit_weights(mocr_engine* e) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (e->committed) throw ArgError{"weights already committed", MOCR_ERR_STATE};
        HIPCHECK(hipSetDevice(e->cfg.device));
        commit_weights(e);
    });
}

void* mocr_stream(mocr_engine* e) { return (e && !e->lanes.empty()) ? (void*)e->lanes[0].ctx.stream : nullptr; }

int mocr_synchronize(mocr_engine* e) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
    });
}

// ---- token constraints ------------------------------------------------------------------------
static int token_set_count(const mocr_engine* e) { return std::max<int>(1, (int)e->tok_sets.size()); }

// one handle per crop (null: every crop MOCR_TOKEN_SET_ALL), each a set this engine has created
static void require_sets(const mocr_engine* e, const int32_t* sets, int n) {
    if (!sets) return;
    const int count = token_set_count(e);
    for (int i = 0; i < n; ++i)
        if (sets[i] < 0 || sets[i] >= count) throw ArgError{"unknown token set handle (mocr_token_set_create)", MOCR_ERR_ARG};
}

// ---- no-repeat n-grams --------------------------------------------------------------------------
// one size per crop (null: every crop 0 = off), each in 0 .. the engine's max_len
static void require_ngram(const mocr_engine* e, const int32_t* ngram, int n) {
    if (!ngram) return;
    for (int i = 0; i < n; ++i)
        if (ngram[i] < 0 || ngram[i] > e->cfg.max_len) throw ArgError{"no_repeat_ngram_size outside 0 .. max_len", MOCR_ERR_ARG};
}

int mocr_token_set_create(mocr_engine* e, const int32_t* ids, int32_t n_ids, int32_t* out_set) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!e->committed) throw ArgError{"weights not committed (mocr_commit_weights)", MOCR_ERR_STATE};
        if (!ids || n_ids <= 0 || !out_set || e->V % 32) throw ArgError{"mocr_token_set_create: bad argument", MOCR_ERR_ARG};
        const size_t words = (size_t)e->V / 32;
        std::vector<uint32_t> bits(words, 0u);
        for (int i = 0; i < n_ids; ++i) {
            if (ids[i] < 0 || ids[i] >= e->V) throw ArgError{"mocr_token_set_create: token id outside the vocabulary", MOCR_ERR_ARG};
            bits[ids[i] >> 5] |= 1u << (ids[i] & 31);
        }
        const int eos = e->cfg.eos_id;       // a recogniser that cannot stop is useless: EOS is in every set
        if (eos >= 0 && eos < e->V) bits[eos >> 5] |= 1u << (eos & 31);
        HIPCHECK(hipSetDevice(e->cfg.device));
        ensure_tok_table(e);
        const auto it = e->tok_index.find(bits);
        if (it != e->tok_index.end()) { *out_set = it->second; return; }
        if ((int)e->tok_sets.size() >= MOCR_MAX_TOKEN_SETS) throw ArgError{"mocr_token_set_create: the set table is full", MOCR_ERR_ARG};
        // a fresh table row: no queued or running batch can hold this handle yet, so the copy races with nothing
        const int h = (int)e->tok_sets.size();
        HIPCHECK(hipMemcpy(e->tok_table + (size_t)h * words, bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
        e->tok_sets.push_back(bits);
        e->tok_index[bits] = h;
        *out_set = h;
    });
}

int mocr_token_set_count(mocr_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return token_set_count(e);
}

// ---- token automata ----------------------------------------------------------------------------
int mocr_automaton_create(mocr_engine* e, const mocr_automaton_desc* d, int32_t* out_handle) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!e->committed) throw ArgError{"weights not committed (mocr_commit_weights)", MOCR_ERR_STATE};
        // (the struct grew by edge_weight and default_next: a caller that passes the short struct gets a hard automaton)
        if (!d || d->struct_size < (int32_t)offsetof(mocr_automaton_desc, edge_weight) || !out_handle || d->n_states < 1 || !d->edge_begin ||
            !d->accepting)
            throw ArgError{"mocr_automaton_create: bad argument", MOCR_ERR_ARG};
        const bool grown = d->struct_size >= (int32_t)sizeof(mocr_automaton_desc);
        const float* const edge_weight = grown ? d->edge_weight : nullptr;
        const int32_t* const default_next = grown ? d->default_next : nullptr;
        const bool soft = edge_weight || default_next;
        const int ns = d->n_states;
        if (d->edge_begin[0] != 0) throw ArgError{"mocr_automaton_create: edge_begin[0] must be 0", MOCR_ERR_ARG};
        for (int s = 0; s < ns; ++s)
            if (d->edge_begin[s + 1] < d->edge_begin[s]) throw ArgError{"mocr_automaton_create: edge_begin is not monotone", MOCR_ERR_ARG};
        const int ne = d->edge_begin[ns];
        if (ne > 0 && (!d->edge_token || !d->edge_next)) throw ArgError{"mocr_automaton_create: edges without their arrays", MOCR_ERR_ARG};
        if ((int)e->aut_first.size() > MOCR_MAX_AUTOMATA || ns > MOCR_MAX_AUTOMATON_STATES - e->aut_n_states ||
            ne > MOCR_MAX_AUTOMATON_EDGES - e->aut_n_edges)
            throw ArgError{"mocr_automaton_create: the automaton tables are full", MOCR_ERR_ARG};
        const int S0 = e->aut_n_states, E0 = e->aut_n_edges;
        std::vector<int> begin((size_t)ns + 1), next((size_t)ne);
        for (int s = 0; s <= ns; ++s) begin[s] = E0 + d->edge_begin[s];
        for (int s = 0; s < ns; ++s)
            for (int i = d->edge_begin[s]; i < d->edge_begin[s + 1]; ++i) {
                const int tok = d->edge_token[i];
                if (tok < 0 || tok >= e->V || tok == e->cfg.eos_id)
                    throw ArgError{"mocr_automaton_create: edge token outside the vocabulary, or EOS", MOCR_ERR_ARG};
                if (i > d->edge_begin[s] && tok <= d->edge_token[i - 1])
                    throw ArgError{"mocr_automaton_create: a state's tokens must be strictly ascending", MOCR_ERR_ARG};
                if (d->edge_next[i] < 0 || d->edge_next[i] >= ns) throw ArgError{"mocr_automaton_create: edge_next outside [0, n_states)", MOCR_ERR_ARG};
                next[i] = S0 + d->edge_next[i];
            }
        std::vector<int> dnext;
        if (edge_weight)
            for (int i = 0; i < ne; ++i)
                if (!std::isfinite(edge_weight[i])) throw ArgError{"mocr_automaton_create: edge_weight must be finite", MOCR_ERR_ARG};
        if (default_next) {
            dnext.resize((size_t)ns);
            for (int s = 0; s < ns; ++s) {
                // (a state number, with or without MOCR_DEFAULT_FALLBACK, or -1; the arena keeps the bit on the global number)
                const int to = default_next[s] < 0 ? default_next[s] : default_next[s] & ~MOCR_DEFAULT_FALLBACK;
                if (to < -1 || to >= ns)
                    throw ArgError{"mocr_automaton_create: default_next outside [0, n_states) and not -1", MOCR_ERR_ARG};
                dnext[s] = to < 0 ? -1 : (S0 + to) | (default_next[s] & MOCR_DEFAULT_FALLBACK);
            }
        }
        HIPCHECK(hipSetDevice(e->cfg.device));
        ensure_automaton_arena(e);
        if (soft) ensure_soft_arena(e);
        // fresh states behind the last automaton's: no queued or running batch can hold this handle yet, so the copies race
        // with nothing (edge_begin[S0] is rewritten with the value it has)
        HIPCHECK(hipMemcpy(e->aut_edge_begin + S0, begin.data(), begin.size() * sizeof(int), hipMemcpyHostToDevice));
        if (ne > 0) {
            HIPCHECK(hipMemcpy(e->aut_edge_token + E0, d->edge_token, (size_t)ne * sizeof(int), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(e->aut_edge_next + E0, next.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice));
        }
        HIPCHECK(hipMemcpy(e->aut_accepting + S0, d->accepting, (size_t)ns, hipMemcpyHostToDevice));
        // (the soft arrays hold 0 / -1 wherever no create has written: nothing to do for an array that did not come)
        if (edge_weight && ne > 0) HIPCHECK(hipMemcpy(e->aut_edge_weight + E0, edge_weight, (size_t)ne * sizeof(float), hipMemcpyHostToDevice));
        if (default_next) HIPCHECK(hipMemcpy(e->aut_default_next + S0, dnext.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice));
        *out_handle = (int32_t)e->aut_first.size();
        e->aut_first.push_back(S0); e->aut_states.push_back(ns); e->aut_soft.push_back(soft ? 1 : 0);
        e->aut_n_states += ns; e->aut_n_edges += ne;
    });
}

int mocr_automaton_count(mocr_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return (int)e->aut_first.size() - 1;
}

int64_t mocr_automaton_state_bytes(mocr_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    int64_t bytes = e->aut_edge_begin ? (int64_t)AUT_ARENA_BYTES : 0;
    if (e->aut_edge_weight) bytes += (int64_t)AUT_SOFT_ARENA_BYTES;
    for (const Lane& L : e->lanes)
    {
        if (L.ctx.aut_state) bytes += 3 * (int64_t)e->Bp * (int64_t)sizeof(int);
        if (L.ctx.hyp_state) bytes += (int64_t)e->Bp * (int64_t)sizeof(int);      // the automaton form of beam search
    }
    return bytes;
}

// ---- one recognise request -----------------------------------------------------------------------
// What a caller may ask for beyond ids and lengths; every mocr_recognize_* symbol is its source kind's implementation with
// some of these null.  The outputs are [n][max_len] rows (x MOCR_ALTERNATIVES / MOCR_POSITION_FIELDS), host or device like
// out_ids; `sets` and `ngram` are host arrays of one int per crop.
struct Request {
    float* out_logp = nullptr;
    int32_t* out_alt_ids = nullptr; float* out_alt_logp = nullptr;     // both or neither
    const int32_t* sets = nullptr;
    const int32_t* ngram = nullptr;
    float* out_pos = nullptr;
    const int32_t* prefix = nullptr;        // host [n][prefix_ld], with prefix_len host [n]: both or neither
    const int32_t* prefix_len = nullptr;
    int32_t prefix_ld = 0;
    // shared encodings (the *_shared entry points): host [rows], the image / region / plane every row decodes (null: row r
    // reads number r), and how many of those the call brings (-1: not said - as many as rows)
    const int32_t* source = nullptr;
    int32_t n_images = -1;
    // beam search (the *_beam entry points; null: greedy): the rows are the crops' beams, K per crop through `source`, and
    // out_score [rows] receives the hypotheses' scores
    const mocr_beam_config* beam = nullptr;
    float* out_score = nullptr;
    // token automata (the *_automaton entry points): host [rows] handles (null: every row MOCR_AUTOMATON_NONE), and [rows]
    // final states, host or device like out_ids
    const int32_t* automata = nullptr;
    int32_t* out_state = nullptr;
    bool beam_soft = false;     // a beam request from the *_beam_soft entry points: its automata may be soft
    // repetition penalty (the *_penalty entry points): host [rows], finite and > 0 (null: every row 1)
    const float* penalty = nullptr;
};

// repetition penalty: one p per row, finite and > 0 (p < 1 rewards repeats and is allowed); beam search takes none
static void require_penalty(const Request& r, int n) {
    if (!r.penalty) return;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(r.penalty[i]) || !(r.penalty[i] > 0.f)) throw ArgError{"repetition_penalty must be finite and > 0", MOCR_ERR_ARG};
    if (r.beam) throw ArgError{"beam search takes no repetition penalty", MOCR_ERR_ARG};
}

// token automata: one handle per row, MOCR_AUTOMATON_NONE or an automaton this engine has created (a beam request comes
// from the *_beam_automaton entry points alone, with its crops' handles expanded to their K rows)
static void require_automata(const mocr_engine* e, const Request& r, int n) {
    if (!r.automata) return;
    const int count = (int)e->aut_first.size();
    for (int i = 0; i < n; ++i)
        if (r.automata[i] < 0 || r.automata[i] >= count) throw ArgError{"unknown automaton handle (mocr_automaton_create)", MOCR_ERR_ARG};
    if (r.beam && !r.beam_soft)     // the *_beam_automaton contract: biases inside a beam's score are the *_beam_soft rule
        for (int i = 0; i < n; ++i)
            if (e->aut_soft[r.automata[i]]) throw ArgError{"beam search takes no soft automaton (edge_weight / default_next)", MOCR_ERR_ARG};
}

// shared encodings: every index names an image of the call, and every image is named by a row
static void require_source(const Request& r, int n) {
    if (!r.source) {
        if (r.n_images >= 0 && r.n_images != n) throw ArgError{"source is null: n_rows must equal the number of images", MOCR_ERR_ARG};
        return;
    }
    if (n < 1) throw ArgError{"n_rows must be positive", MOCR_ERR_ARG};
    if (r.n_images < 1) throw ArgError{"the number of images must be positive", MOCR_ERR_ARG};
    std::vector<char> named((size_t)r.n_images, 0);
    for (int i = 0; i < n; ++i) {
        if (r.source[i] < 0 || r.source[i] >= r.n_images) throw ArgError{"source index outside [0, number of images)", MOCR_ERR_ARG};
        named[r.source[i]] = 1;
    }
    if (std::find(named.begin(), named.end(), 0) != named.end()) throw ArgError{"an image that no row names", MOCR_ERR_ARG};
}

// forced prefixes: per crop 0 .. gen_len - 1 tokens of the vocabulary, EOS as the last one only (gen_len: the call's generate(max_length))
static void require_prefix(const mocr_engine* e, const Request& r, int n, int gen_len) {
    if ((r.prefix == nullptr) != (r.prefix_len == nullptr)) throw ArgError{"prefix and prefix_len must be both null or both set", MOCR_ERR_ARG};
    if (!r.prefix) return;
    for (int i = 0; i < n; ++i) {
        const int P = r.prefix_len[i];
        if (P < 0 || P > gen_len - 1 || P > r.prefix_ld) throw ArgError{"prefix_len outside 0 .. generate(max_length) - 1, or above prefix_ld", MOCR_ERR_ARG};
        const int32_t* p = r.prefix + (size_t)i * r.prefix_ld;
        for (int k = 0; k < P; ++k) {
            if (p[k] < 0 || p[k] >= e->V) throw ArgError{"prefix token outside the vocabulary", MOCR_ERR_ARG};
            if (p[k] == e->cfg.eos_id && k + 1 < P) throw ArgError{"EOS may only be the last token of a prefix", MOCR_ERR_ARG};
        }
    }
}

// The checks of a request, in the order the entry points have always made them: the alternatives pair, then - for the
// entry points that take crops - require_ready, then the per-crop arrays.
enum class Ready { unchecked, any_n, max_batch };
static void validate_request(mocr_engine* e, const Request& r, int n, Ready ready, int gen_len) {
    if ((r.out_alt_ids == nullptr) != (r.out_alt_logp == nullptr))
        throw ArgError{"out_alt_ids and out_alt_logp must be both null or both set", MOCR_ERR_ARG};
    if (ready != Ready::unchecked) require_ready(e, n, ready == Ready::max_batch);
    require_source(r, n);
    require_sets(e, r.sets, n);
    require_ngram(e, r.ngram, n);
    require_prefix(e, r, n, gen_len);
    require_automata(e, r, n);
    require_penalty(r, n);
}

// rows [base, base + n) of a per-crop array whose default is `dflt`, for the job that decodes them (empty: all default)
static std::vector<int32_t> slice_rows(const int32_t* v, size_t base, int n, int32_t dflt) {
    if (v && std::any_of(v + base, v + base + n, [dflt](int32_t x) { return x != dflt; })) return {v + base, v + base + n};
    return {};
}

// The one place a request and a row range become a job's optional outputs and per-crop vectors.
static void slice_job(Job& j, const Request& r, size_t base, int n, int max_len) {
    const size_t L = (size_t)max_len;
    j.out_logp = r.out_logp ? r.out_logp + base * L : nullptr;
    j.out_alt_ids = r.out_alt_ids ? r.out_alt_ids + base * L * MOCR_ALTERNATIVES : nullptr;
    j.out_alt_logp = r.out_alt_logp ? r.out_alt_logp + base * L * MOCR_ALTERNATIVES : nullptr;
    j.out_pos = r.out_pos ? r.out_pos + base * L * MOCR_POSITION_FIELDS : nullptr;
    j.beam = mocr_beam_config{}; j.out_score = nullptr;
    if (r.beam) {       // a crop's K rows stay in one job: the callers cut a beam request at multiples of K only
        if (base % r.beam->num_beams || n % r.beam->num_beams) throw ArgError{"a beam job is cut at multiples of num_beams", MOCR_ERR_STATE};
        j.beam = *r.beam; j.out_score = r.out_score + base;
    }
    j.sets = slice_rows(r.sets, base, n, MOCR_TOKEN_SET_ALL);
    j.ngram = slice_rows(r.ngram, base, n, 0);
    j.automata = slice_rows(r.automata, base, n, MOCR_AUTOMATON_NONE);
    j.out_state = r.out_state ? r.out_state + base : nullptr;
    j.penalty.clear();
    if (r.penalty && std::any_of(r.penalty + base, r.penalty + base + n, [](float p) { return p != 1.f; }))
        j.penalty.assign(r.penalty + base, r.penalty + base + n);
    j.prefix_len = slice_rows(r.prefix_len, base, n, 0);
    j.prefix.clear(); j.prefix_ld = 0;
    if (!j.prefix_len.empty()) {
        j.prefix_ld = r.prefix_ld;
        j.prefix.assign(r.prefix + base * (size_t)r.prefix_ld, r.prefix + (base + n) * (size_t)r.prefix_ld);
    }
    // shared encodings: the job brings the distinct sources of its own rows, in ascending order (`planes`: their numbers in
    // the call - the caller of slice_job makes them the job's planes), and its rows name them by their place in that list
    j.n_src = n; j.src_of_row.clear(); j.planes.clear();
    if (r.source) {
        j.planes.assign(r.source + base, r.source + base + n);
        std::sort(j.planes.begin(), j.planes.end());
        j.planes.erase(std::unique(j.planes.begin(), j.planes.end()), j.planes.end());
        j.n_src = (int)j.planes.size();
        j.src_of_row.resize((size_t)n);
        for (int i = 0; i < n; ++i)
            j.src_of_row[i] = (int32_t)(std::lower_bound(j.planes.begin(), j.planes.end(), r.source[base + i]) - j.planes.begin());
    }
}

// the exported twins' arguments as a request (the device entry points pass untyped pointers)
static Request request_of(void* out_logp = nullptr, void* out_alt_ids = nullptr, void* out_alt_logp = nullptr,
                          const int32_t* sets = nullptr, const int32_t* ngram = nullptr, void* out_pos = nullptr,
                          const int32_t* prefix = nullptr, const int32_t* prefix_len = nullptr, int32_t prefix_ld = 0,
                          const int32_t* source = nullptr, int32_t n_images = -1) {
    Request r;
    r.source = source; r.n_images = n_images;
    r.out_logp = static_cast<float*>(out_logp);
    r.out_alt_ids = static_cast<int32_t*>(out_alt_ids); r.out_alt_logp = static_cast<float*>(out_alt_logp);
    r.sets = sets; r.ngram = ngram;
    r.out_pos = static_cast<float*>(out_pos);
    r.prefix = prefix; r.prefix_len = prefix_len; r.prefix_ld = prefix_ld;
    return r;
}

// ... and a request with the two arguments the *_automaton twins add
static Request with_automata(Request r, const int32_t* automata, void* out_state) {
    r.automata = automata; r.out_state = static_cast<int32_t*>(out_state);
    return r;
}

// ... and with the one the *_penalty twins add
static Request with_penalty(Request r, const float* penalty) {
    r.penalty = penalty;
    return r;
}

static int recognize_device(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len, const Request& req) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        validate_request(e, req, n, Ready::max_batch, e->gen_max_len);
        if (!d_gray || !d_out_ids || !d_out_len) throw ArgError{"null device pointer", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        Job j;
        j.src = reinterpret_cast<const uint8_t*>(d_gray); j.src_host = false;
        j.n = n; j.max_len = e->gen_max_len;
        j.out_ids = reinterpret_cast<int32_t*>(d_out_ids); j.out_len = reinterpret_cast<int32_t*>(d_out_len); j.out_host = false;
        slice_job(j, req, 0, n, e->cfg.max_len);
        submit(e, j);
    });
}

int mocr_recognize_device_positions(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len,
                                    void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets,
                                    const int32_t* ngram, void* d_out_pos) {
    return recognize_device(e, d_gray, n, d_out_ids, d_out_len, request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp, sets, ngram, d_out_pos));
}

int mocr_recognize_device_prefix(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len, void* d_out_logp,
                                 void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets, const int32_t* ngram, void* d_out_pos,
                                 const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld) {
    return recognize_device(e, d_gray, n, d_out_ids, d_out_len,
                            request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp, sets, ngram, d_out_pos, prefix, prefix_len, prefix_ld));
}

int mocr_recognize_device_shared(mocr_engine* e, const void* d_gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                 void* d_out_ids, void* d_out_len, void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp,
                                 const int32_t* sets, const int32_t* ngram, void* d_out_pos, const int32_t* prefix,
                                 const int32_t* prefix_len, int32_t prefix_ld) {
    return recognize_device(e, d_gray, n_rows, d_out_ids, d_out_len,
                            request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp, sets, ngram, d_out_pos, prefix, prefix_len, prefix_ld,
                                       source, n_planes));
}

int mocr_recognize_device_automaton(mocr_engine* e, const void* d_gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                    void* d_out_ids, void* d_out_len, void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp,
                                    const int32_t* sets, const int32_t* ngram, void* d_out_pos, const int32_t* prefix,
                                    const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, void* d_out_state) {
    return recognize_device(e, d_gray, n_rows, d_out_ids, d_out_len,
                            with_automata(request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp, sets, ngram, d_out_pos, prefix, prefix_len,
                                                     prefix_ld, source, n_planes), automata, d_out_state));
}

int mocr_recognize_device_penalty(mocr_engine* e, const void* d_gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                  void* d_out_ids, void* d_out_len, void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp,
                                  const int32_t* sets, const int32_t* ngram, void* d_out_pos, const int32_t* prefix,
                                  const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, void* d_out_state,
                                  const float* penalty) {
    return recognize_device(e, d_gray, n_rows, d_out_ids, d_out_len,
                            with_penalty(with_automata(request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp, sets, ngram, d_out_pos, prefix,
                                                                  prefix_len, prefix_ld, source, n_planes), automata, d_out_state), penalty));
}

int mocr_recognize_device_norepeat(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len,
                                   void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets,
                                   const int32_t* ngram) {
    return recognize_device(e, d_gray, n, d_out_ids, d_out_len, request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp, sets, ngram));
}

int mocr_recognize_device_constrained(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len,
                                      void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets) {
    return recognize_device(e, d_gray, n, d_out_ids, d_out_len, request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp, sets));
}

int mocr_recognize_device_alts(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len, void* d_out_logp,
                               void* d_out_alt_ids, void* d_out_alt_logp) {
    return recognize_device(e, d_gray, n, d_out_ids, d_out_len, request_of(d_out_logp, d_out_alt_ids, d_out_alt_logp));
}

int mocr_recognize_device_scored(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len, void* d_out_logp) {
    return recognize_device(e, d_gray, n, d_out_ids, d_out_len, request_of(d_out_logp));
}

int mocr_recognize_device(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len) {
    return recognize_device(e, d_gray, n, d_out_ids, d_out_len, Request{});
}

static void recognize_host_chunks(mocr_engine* e, const uint8_t* images, int n, int h, int w, int64_t row_stride,
                                  int64_t image_stride, int channels, int max_len, int32_t* out_ids, int32_t* out_len,
                                  const Request& req) {
    const int IMG = e->cfg.image_size;
    if (h != IMG || w != IMG)
        throw ArgError{"crops must be image_size x image_size (resize with PIL BILINEAR on the caller side)", MOCR_ERR_UNSUPPORTED};
    if (channels != 1 && channels != 3) throw ArgError{"channels must be 1 (L) or 3 (RGB)", MOCR_ERR_ARG};
    if (!images || !out_ids || !out_len) throw ArgError{"null pointer", MOCR_ERR_ARG};
    if (max_len < 2 || max_len > e->cfg.max_len) throw ArgError{"bad max_len override", MOCR_ERR_ARG};
    for (int base = 0; base < n; base += e->cfg.max_batch) {
        Job j;
        // (a job that shares finds its planes by their numbers in the call: slice_job's `planes`)
        j.src = images + (req.source ? 0 : (size_t)base * image_stride); j.src_host = true; j.channels = channels;
        j.row_stride = row_stride; j.image_stride = image_stride;
        j.n = std::min(e->cfg.max_batch, n - base); j.max_len = max_len;
        j.out_ids = out_ids + (size_t)base * e->cfg.max_len; j.out_len = out_len + base; j.out_host = true;
        slice_job(j, req, (size_t)base, j.n, e->cfg.max_len);
        e->pending.push_back(j);
    }
    drive(e);
}

int mocr_recognize(mocr_engine* e, const uint8_t* images, int32_t n, int32_t h, int32_t w, int64_t row_stride,
                   int64_t image_stride, int32_t channels, int32_t* out_ids, int32_t* out_len) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        require_ready(e, n, false);
        HIPCHECK(hipSetDevice(e->cfg.device));
        recognize_host_chunks(e, images, n, h, w, row_stride, image_stride, channels, e->gen_max_len, out_ids, out_len, Request{});
    });
}

static int recognize_gray_host(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                               int32_t* out_len, const Request& req) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        validate_request(e, req, n, Ready::any_n, max_len_override);
        HIPCHECK(hipSetDevice(e->cfg.device));
        const int IMG = e->cfg.image_size;
        recognize_host_chunks(e, gray, n, IMG, IMG, IMG, (int64_t)IMG * IMG, 1, max_len_override, out_ids, out_len, req);
    });
}

int mocr_recognize_gray_host_positions(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                       int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                       const int32_t* sets, const int32_t* ngram, float* out_pos) {
    return recognize_gray_host(e, gray, n, max_len_override, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos));
}

int mocr_recognize_gray_host_prefix(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                    int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets,
                                    const int32_t* ngram, float* out_pos, const int32_t* prefix, const int32_t* prefix_len,
                                    int32_t prefix_ld) {
    return recognize_gray_host(e, gray, n, max_len_override, out_ids, out_len,
                               request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld));
}

int mocr_recognize_gray_host_shared(mocr_engine* e, const uint8_t* gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                    int32_t max_len_override, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                    float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos,
                                    const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld) {
    return recognize_gray_host(e, gray, n_rows, max_len_override, out_ids, out_len,
                               request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld,
                                          source, n_planes));
}

int mocr_recognize_gray_host_automaton(mocr_engine* e, const uint8_t* gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                       int32_t max_len_override, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                       float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos,
                                       const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata,
                                       int32_t* out_state) {
    return recognize_gray_host(e, gray, n_rows, max_len_override, out_ids, out_len,
                               with_automata(request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len,
                                                        prefix_ld, source, n_planes), automata, out_state));
}

int mocr_recognize_gray_host_penalty(mocr_engine* e, const uint8_t* gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                     int32_t max_len_override, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                     float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos,
                                     const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata,
                                     int32_t* out_state, const float* penalty) {
    return recognize_gray_host(e, gray, n_rows, max_len_override, out_ids, out_len,
                               with_penalty(with_automata(request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len,
                                                                     prefix_ld, source, n_planes), automata, out_state), penalty));
}

int mocr_recognize_gray_host_norepeat(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                      int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                      const int32_t* sets, const int32_t* ngram) {
    return recognize_gray_host(e, gray, n, max_len_override, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram));
}

int mocr_recognize_gray_host_constrained(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                         int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                         const int32_t* sets) {
    return recognize_gray_host(e, gray, n, max_len_override, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets));
}

int mocr_recognize_gray_host_alts(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                  int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp) {
    return recognize_gray_host(e, gray, n, max_len_override, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp));
}

int mocr_recognize_gray_host_scored(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                    int32_t* out_len, float* out_logp) {
    return recognize_gray_host(e, gray, n, max_len_override, out_ids, out_len, request_of(out_logp));
}

int mocr_recognize_gray_host(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                             int32_t* out_len) {
    return recognize_gray_host(e, gray, n, max_len_override, out_ids, out_len, Request{});
}

// Host pixels uploaded once (an image, or a whole page several crops are cut from) ...
struct PrepSource { const uint8_t* data; int h, w; int64_t row_stride; int ch; int bgr; int rot; };
// ... and what one crop reads of its source: the rectangle [x, x+w) x [y, y+h), then rotated (MOCR_ROTATE_*)
struct PrepView { int source, x, y, w, h, rot; };

static PrepSource source_of(const mocr_image& im) {
    const int ch = im.channels == MOCR_CHANNELS_BGR ? 3 : im.channels;
    if (!im.data || im.height < 1 || im.width < 1 || im.height > 16384 || im.width > 16384 || (ch != 1 && ch != 3) ||
        im.row_stride < (int64_t)im.width * ch)
        throw ArgError{"bad image descriptor (channels must be 1 = L, 3 = RGB or MOCR_CHANNELS_BGR)", MOCR_ERR_ARG};
    if (im.rotate != MOCR_ROTATE_NONE && im.rotate != MOCR_ROTATE_90_CW && im.rotate != MOCR_ROTATE_90_CCW)
        throw ArgError{"bad image descriptor (rotate must be MOCR_ROTATE_NONE, _90_CW or _90_CCW)", MOCR_ERR_ARG};
    return PrepSource{im.data, im.height, im.width, im.row_stride, ch, im.channels == MOCR_CHANNELS_BGR ? 1 : 0, im.rotate};
}

// L conversion + Pillow-exact BILINEAR resize of the views (any sizes) into d_out [views][IMG][IMG] u8 on the
// device; synchronous (lane 0's stream).  Every source is uploaded once, however many views read it: the crops of
// a page's detected regions are cut ON THE DEVICE (descriptor = offset + page stride), not copied out on the host.
// prep_enqueue packs the sources into pinned buffer `slot`, and enqueues H2D + the two resize launches on the engine's
// preparation stream; it does NOT wait for them.  Device scratch (packed sources, horizontal-pass planes, descriptors,
// coefficient tables) is reused from call to call: everything runs on the ONE preparation stream, in order.  The pinned
// buffer of a slot may be repacked only once the copy that reads it has finished (the caller's business).
struct PrepHold { std::vector<ResizeDesc> descs; std::vector<int> coef, bounds; };     // host sources of a pass's small uploads: alive until it has run
static void prep_enqueue(mocr_engine* e, const std::vector<PrepSource>& srcs, const PrepView* views, int n, uint8_t* d_out, int slot, bool prof,
                         PrepHold& hold) {
    const int IMG = e->cfg.image_size;
    if (n > 4096) throw ArgError{"prep_enqueue: at most 4096 crops per pass", MOCR_ERR_ARG};   // bounded scratch and grid.y
    if (IMG != 224) throw ArgError{"device preprocessing is instantiated for image_size 224", MOCR_ERR_UNSUPPORTED};
    std::vector<ResizeDesc>& descs = hold.descs;
    std::vector<int>&coef = hold.coef, &bounds = hold.bounds;
    descs.assign(n, ResizeDesc{});
    coef.clear(); bounds.clear();
    std::map<int, std::pair<int, int>> placed;        // input size -> (coef offset, bounds offset) in this call's buffers
    std::map<int, long long> src_off;                 // sources this pass reads -> byte offset in the packed upload
    size_t src_bytes = 0, tmp_bytes = 0;
    int max_h = 0;
    auto place = [&](int in_size, int& k_off, int& b_off, int& ks) {
        if (in_size == IMG) { k_off = b_off = ks = 0; return; }           // Pillow skips a pass whose size is unchanged
        auto it = e->rs_tables.find(in_size);
        if (it == e->rs_tables.end()) it = e->rs_tables.emplace(in_size, make_resample_table(in_size, IMG)).first;
        const ResampleTable& t = it->second;
        auto pl = placed.find(in_size);
        if (pl == placed.end()) {
            pl = placed.emplace(in_size, std::make_pair((int)coef.size(), (int)bounds.size())).first;
            coef.insert(coef.end(), t.kk.begin(), t.kk.end());
            bounds.insert(bounds.end(), t.bounds.begin(), t.bounds.end());
        }
        k_off = pl->second.first; b_off = pl->second.second; ks = t.ksize;
    };
    for (int i = 0; i < n; ++i) {
        const PrepView& v = views[i];
        if (v.source < 0 || v.source >= (int)srcs.size()) throw ArgError{"view of an unknown source", MOCR_ERR_ARG};
        const PrepSource& sc = srcs[v.source];
        if (v.w < 1 || v.h < 1 || v.x < 0 || v.y < 0 || v.x + v.w > sc.w || v.y + v.h > sc.h)
            throw ArgError{"view outside its source image", MOCR_ERR_ARG};
        auto so = src_off.find(v.source);
        if (so == src_off.end()) {
            so = src_off.emplace(v.source, (long long)src_bytes).first;
            src_bytes += (size_t)sc.h * sc.w * sc.ch;
        }
        ResizeDesc& d = descs[i];
        d.channels = sc.ch; d.bgr = sc.bgr;
        const int stride = sc.w * sc.ch;                        // the packed copy has no row padding
        const long long origin = so->second + ((long long)v.y * sc.w + v.x) * sc.ch;
        if (v.rot == MOCR_ROTATE_90_CW) {                       // R[y'][x'] = S[h - 1 - x'][y']   (np.rot90(k = -1))
            d.h = v.w; d.w = v.h; d.row_step = sc.ch; d.pix_step = -stride;
            d.src_off = origin + (long long)(v.h - 1) * stride;
        } else if (v.rot == MOCR_ROTATE_90_CCW) {               // R[y'][x'] = S[x'][w - 1 - y']   (np.rot90(k = 1))
            d.h = v.w; d.w = v.h; d.row_step = -sc.ch; d.pix_step = stride;
            d.src_off = origin + (long long)(v.w - 1) * sc.ch;
        } else {
            d.h = v.h; d.w = v.w; d.row_step = stride; d.pix_step = sc.ch;
            d.src_off = origin;
        }
        d.tmp_off = (long long)tmp_bytes;
        tmp_bytes += (size_t)d.h * IMG;
        place(d.w, d.kx_off, d.bx_off, d.ksx);
        place(d.h, d.ky_off, d.by_off, d.ksy);
        max_h = std::max(max_h, d.h);
    }
    // pack the pixel rows of every source (drops the callers' row padding) into the pinned staging buffer, the
    // sources dealt to a few host threads by bytes (2048 crops of 224 x 224 x 3 are 300 MB: ~50 ms on one core)
    uint8_t* const packed = (uint8_t*)e->grow_pinned(slot, src_bytes);
    {
        std::vector<std::pair<int, long long>> items(src_off.begin(), src_off.end());
        auto pack_range = [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i) {
                const PrepSource& sc = srcs[items[i].first];
                uint8_t* dst = packed + items[i].second;
                const size_t rowb = (size_t)sc.w * sc.ch;
                if ((int64_t)rowb == sc.row_stride) memcpy(dst, sc.data, rowb * sc.h);
                else
                    for (int y = 0; y < sc.h; ++y) memcpy(dst + (size_t)y * rowb, sc.data + (size_t)y * sc.row_stride, rowb);
            }
        };
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const size_t nthr = std::min<size_t>({(size_t)8, (size_t)hw, items.size(), src_bytes / (4u << 20) + 1});
        if (nthr <= 1) pack_range(0, items.size());
        else {
            std::vector<std::thread> pool;
            const size_t per = (items.size() + nthr - 1) / nthr;
            for (size_t k = 0; k < nthr; ++k) {
                const size_t i0 = k * per, i1 = std::min(items.size(), i0 + per);
                if (i0 < i1) pool.emplace_back(pack_range, i0, i1);
            }
            for (auto& th : pool) th.join();
        }
    }
    uint8_t* d_src = (uint8_t*)e->grow(e->rs_src, src_bytes);
    uint8_t* d_tmp = (uint8_t*)e->grow(e->rs_tmp, tmp_bytes);
    ResizeDesc* d_desc = (ResizeDesc*)e->grow(e->rs_desc, descs.size() * sizeof(ResizeDesc));
    int* d_coef = (int*)e->grow(e->rs_coef, std::max<size_t>(coef.size(), 1) * sizeof(int));
    int* d_bounds = (int*)e->grow(e->rs_bounds, std::max<size_t>(bounds.size(), 1) * sizeof(int));
    hipStream_t st = e->prep_stream;
    HIPCHECK(hipMemcpyAsync(d_src, packed, src_bytes, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_desc, descs.data(), descs.size() * sizeof(ResizeDesc), hipMemcpyHostToDevice, st));
    if (!coef.empty()) HIPCHECK(hipMemcpyAsync(d_coef, coef.data(), coef.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!bounds.empty()) HIPCHECK(hipMemcpyAsync(d_bounds, bounds.data(), bounds.size() * sizeof(int), hipMemcpyHostToDevice, st));
    constexpr int ROWS = 8;
    hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr;
    if (prof) { t0 = e->get_event(); t1 = e->get_event(); t2 = e->get_event(); HIPCHECK(hipEventRecord(t0, st)); }
    hipLaunchKernelGGL((resize_h_kernel<224, ROWS>), dim3((max_h + ROWS - 1) / ROWS, n), dim3(256), 0, st, d_src, d_desc, d_coef, d_bounds, d_tmp);
    HIPCHECK(hipGetLastError());
    if (prof) HIPCHECK(hipEventRecord(t1, st));
    hipLaunchKernelGGL((resize_v_kernel<224, ROWS>), dim3(224 / ROWS, n), dim3(256), 0, st, d_tmp, d_desc, d_coef, d_bounds, d_out);
    HIPCHECK(hipGetLastError());
    if (prof) {
        HIPCHECK(hipEventRecord(t2, st));
        e->recs.push_back(ProfRec{e->kid("resize_h"), t0, t1, 0, (double)src_bytes + (double)tmp_bytes});
        hipEvent_t t1b = e->get_event();         // (a record owns both of its events)
        HIPCHECK(hipEventRecord(t1b, st));
        e->recs.push_back(ProfRec{e->kid("resize_v"), t1b, t2, 0, (double)tmp_bytes + (double)n * IMG * IMG});
    }
}

// Synchronous form (test hook mocr_preprocess, small calls): L conversion + Pillow-exact BILINEAR resize of the views
// into d_out [views][IMG][IMG] u8 on the device.
static void preprocess_views(mocr_engine* e, const std::vector<PrepSource>& srcs, const PrepView* views, int n, uint8_t* d_out) {
    const size_t plane = (size_t)e->cfg.image_size * e->cfg.image_size;
    PrepHold hold;
    for (int b = 0; b < n; b += 4096) {
        prep_enqueue(e, srcs, views + b, std::min(4096, n - b), d_out + (size_t)b * plane, 0, e->prof_on, hold);
        HIPCHECK(hipStreamSynchronize(e->prep_stream));     // the staging buffer and the descriptors are reused by the next pass
    }
}

static void preprocess_images(mocr_engine* e, const mocr_image* imgs, int n, uint8_t* d_out) {
    std::vector<PrepSource> srcs(n);
    std::vector<PrepView> views(n);
    for (int i = 0; i < n; ++i) {
        srcs[i] = source_of(imgs[i]);
        views[i] = PrepView{i, 0, 0, srcs[i].w, srcs[i].h, srcs[i].rot};
    }
    preprocess_views(e, srcs, views.data(), n, d_out);
}

// THE host entry points' engine: crops (views of host sources) -> ids.  The views are cut into chunks of max_batch
// rows = one decode job each.  A producer thread prepares chunk k + 1 (pack into the other pinned buffer, H2D, resize, on
// the preparation stream) while the lanes decode chunk k; a job's lane stream waits ON THE DEVICE for its chunk's event,
// so the host never blocks on a preparation.  r02 prepared ALL crops, synchronised, and only then started to decode.
static void prepare_and_decode(mocr_engine* e, const std::vector<PrepSource>& srcs, const PrepView* views, int n, int32_t* out_ids,
                               int32_t* out_len, const Request& req) {
    const size_t plane = (size_t)e->cfg.image_size * e->cfg.image_size;
    const int Kb = req.beam ? req.beam->num_beams : 1;       // (a beam request is cut at multiples of K: a crop's beams stay together)
    const int C = std::min(e->cfg.max_batch, 4096) / Kb * Kb, nchunks = (n + C - 1) / C;
    // `n` decode rows over the views (req.source; without it row r reads view r).  A chunk prepares the views its own rows
    // name, once each: the planes of its job.
    struct Chunk { int plane0 = 0; std::vector<PrepView> own; const PrepView* views = nullptr; Job job; };
    std::vector<Chunk> chunks(nchunks);
    int total_planes = 0;
    for (int k = 0; k < nchunks; ++k) {
        Chunk& c = chunks[k];
        Job& j = c.job;
        j.src_host = false; j.channels = 1;
        j.row_stride = e->cfg.image_size; j.image_stride = (int64_t)plane;
        j.n = std::min(C, n - k * C); j.max_len = e->gen_max_len;
        j.out_ids = out_ids + (size_t)k * C * e->cfg.max_len; j.out_len = out_len + (size_t)k * C; j.out_host = true;
        slice_job(j, req, (size_t)k * C, j.n, e->cfg.max_len);
        c.views = views + (size_t)k * C;
        if (req.source) {
            for (int32_t v : j.planes) c.own.push_back(views[v]);
            c.views = c.own.data();
            j.planes.clear();       // prepared side by side, in that order
        }
        c.plane0 = total_planes;
        total_planes += j.n_src;
    }
    uint8_t* const d_gray = (uint8_t*)e->grow(e->rs_gray, (size_t)total_planes * plane);
    auto chunk_out = [&](int k) { return d_gray + (size_t)chunks[k].plane0 * plane; };
    auto push_job = [&](int k, hipEvent_t ev) {
        Job& j = chunks[k].job;
        j.wait_ev = ev;
        j.src = chunk_out(k);
        e->pending.push_back(j);
    };
    std::vector<PrepHold> holds(nchunks);
    if (nchunks == 1 || e->prof_on) {              // nothing to overlap (or an instrumented pass: one thread records the events)
        for (int k = 0; k < nchunks; ++k) {
            prep_enqueue(e, srcs, chunks[k].views, chunks[k].job.n_src, chunk_out(k), 0, e->prof_on, holds[k]);
            HIPCHECK(hipStreamSynchronize(e->prep_stream));
            push_job(k, nullptr);
        }
        drive(e);
        return;
    }
    std::vector<hipEvent_t> ev(nchunks, nullptr);
    for (auto& x : ev) HIPCHECK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    auto cleanup = [&] {
        (void)hipStreamSynchronize(e->prep_stream);
        for (auto x : ev) if (x) (void)hipEventDestroy(x);
    };
    run_prep_pipeline(
        nchunks,
        [&](int k) {                                   // producer thread: pinned buffer k & 1 is free once chunk k - 2's copy has run
            if (k == 0) HIPCHECK(hipSetDevice(e->cfg.device));
            if (k >= 2) HIPCHECK(hipEventSynchronize(ev[k - 2]));
        },
        [&](int k) {                                   // producer thread
            prep_enqueue(e, srcs, chunks[k].views, chunks[k].job.n_src, chunk_out(k), k & 1, false, holds[k]);
            HIPCHECK(hipEventRecord(ev[k], e->prep_stream));
        },
        [&](int k) { push_job(k, ev[k]); },            // calling thread
        [&] { return (e->cfg.dtype == MOCR_BF16) ? pump_once<bf16_t>(e) : pump_once<float>(e); },
        [&] {                                          // either side failed: nothing stays queued, nothing stays in flight
            e->pending.clear();
            for (auto& L : e->lanes) { L.active = false; L.jobs.clear(); (void)hipStreamSynchronize(L.ctx.stream); }
            cleanup();
        });
    for (auto& L : e->lanes) HIPCHECK(hipStreamSynchronize(L.ctx.stream));
    cleanup();
}

int mocr_preprocess(mocr_engine* e, const mocr_image* images, int32_t n, uint8_t* out_gray) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!images || !out_gray || n < 1) throw ArgError{"bad argument", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->bind(0);
        const size_t plane = (size_t)e->cfg.image_size * e->cfg.image_size;
        uint8_t* d_gray = (uint8_t*)e->grow(e->rs_gray, (size_t)n * plane);
        preprocess_images(e, images, n, d_gray);
        HIPCHECK(hipMemcpy(out_gray, d_gray, (size_t)n * plane, hipMemcpyDeviceToHost));
        e->unbind(0);
    });
}

static int recognize_images(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len, const Request& req) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        validate_request(e, req, n, Ready::any_n, e->gen_max_len);
        if (!images || !out_ids || !out_len) throw ArgError{"null pointer", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        const int n_images = req.source ? req.n_images : n;      // n: decode rows
        std::vector<PrepSource> srcs(n_images);
        std::vector<PrepView> views(n_images);
        for (int i = 0; i < n_images; ++i) {
            srcs[i] = source_of(images[i]);
            views[i] = PrepView{i, 0, 0, srcs[i].w, srcs[i].h, srcs[i].rot};
        }
        prepare_and_decode(e, srcs, views.data(), n, out_ids, out_len, req);
    });
}

int mocr_recognize_images_positions(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                    float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets,
                                    const int32_t* ngram, float* out_pos) {
    return recognize_images(e, images, n, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos));
}

int mocr_recognize_images_prefix(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                 float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                 float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld) {
    return recognize_images(e, images, n, out_ids, out_len,
                            request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld));
}

int mocr_recognize_images_shared(mocr_engine* e, const mocr_image* images, int32_t n_images, int32_t n_rows, const int32_t* source,
                                 int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                 const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                 const int32_t* prefix_len, int32_t prefix_ld) {
    return recognize_images(e, images, n_rows, out_ids, out_len,
                            request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld, source,
                                       n_images));
}

int mocr_recognize_images_automaton(mocr_engine* e, const mocr_image* images, int32_t n_images, int32_t n_rows, const int32_t* source,
                                    int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                    const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                    const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, int32_t* out_state) {
    return recognize_images(e, images, n_rows, out_ids, out_len,
                            with_automata(request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld,
                                                     source, n_images), automata, out_state));
}

int mocr_recognize_images_penalty(mocr_engine* e, const mocr_image* images, int32_t n_images, int32_t n_rows, const int32_t* source,
                                  int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                  const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                  const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, int32_t* out_state,
                                  const float* penalty) {
    return recognize_images(e, images, n_rows, out_ids, out_len,
                            with_penalty(with_automata(request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len,
                                                                  prefix_ld, source, n_images), automata, out_state), penalty));
}

int mocr_recognize_images_norepeat(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                   float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets,
                                   const int32_t* ngram) {
    return recognize_images(e, images, n, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram));
}

int mocr_recognize_images_constrained(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                      float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets) {
    return recognize_images(e, images, n, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets));
}

int mocr_recognize_images_alts(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                               float* out_logp, int32_t* out_alt_ids, float* out_alt_logp) {
    return recognize_images(e, images, n, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp));
}

int mocr_recognize_images_scored(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                 float* out_logp) {
    return recognize_images(e, images, n, out_ids, out_len, request_of(out_logp));
}

int mocr_recognize_images(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len) {
    return recognize_images(e, images, n, out_ids, out_len, Request{});
}

// The crop a detected text region gets (src/ui/main_window.py:9530-9540): its bounding box grown by
// int(max(w, h) * 0.08) on every side, clipped to the page; false when no more than a 1-pixel sliver is left
// (the reference then returns '' without calling the recogniser).
static bool padded_region(const mocr_region& r, int page_h, int page_w, PrepView& v) {
    if (r.width < 0 || r.height < 0) throw ArgError{"region with a negative size", MOCR_ERR_ARG};
    const int pad = (int)((double)std::max(r.width, r.height) * 0.08);
    const long long x1 = std::max<long long>((long long)r.x - pad, 0), y1 = std::max<long long>((long long)r.y - pad, 0);
    const long long x2 = std::min<long long>((long long)r.x + r.width + pad, page_w), y2 = std::min<long long>((long long)r.y + r.height + pad, page_h);
    if (x2 - x1 <= 1 || y2 - y1 <= 1) return false;
    v.x = (int)x1; v.y = (int)y1; v.w = (int)(x2 - x1); v.h = (int)(y2 - y1);
    return true;
}

// n_rows decode rows over n_regions regions (req.source; without it n_rows == n_regions and row r reads region r): the per-row
// arrays of the request and every output go by row.
static int recognize_regions(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions, int32_t n_regions,
                             int32_t n_rows, int32_t* out_ids, int32_t* out_len, const Request& req) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        validate_request(e, req, std::max(n_rows, 0), Ready::unchecked, e->gen_max_len);
        if (!e->committed) throw ArgError{"weights not committed (mocr_commit_weights)", MOCR_ERR_STATE};
        if (!pages || n_pages < 1 || n_regions < 0 || n_rows < 0 || (n_rows > 0 && (!regions || !out_ids || !out_len)))
            throw ArgError{"bad argument", MOCR_ERR_ARG};
        if (n_rows == 0) return;
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        std::vector<PrepSource> srcs(n_pages);
        for (int i = 0; i < n_pages; ++i) srcs[i] = source_of(pages[i]);
        std::vector<PrepView> views;
        std::vector<int> view_of(n_regions, -1);        // region -> its place among the recognised crops (-1: sliver)
        for (int i = 0; i < n_regions; ++i) {
            const mocr_region& r = regions[i];
            if (r.page < 0 || r.page >= n_pages) throw ArgError{"region of an unknown page", MOCR_ERR_ARG};
            PrepView v{r.page, 0, 0, 0, 0, MOCR_ROTATE_NONE};
            if (!padded_region(r, srcs[r.page].h, srcs[r.page].w, v)) continue;
            view_of[i] = (int)views.size();
            views.push_back(v);
        }
        std::vector<int> where(n_rows, -1);             // row -> its row among the recognised rows (-1: a sliver's)
        std::vector<int32_t> view_src;                  // the recognised rows' crops
        std::vector<int32_t> view_sets;                 // ... token sets
        std::vector<int32_t> view_ngram;                // ... and no-repeat n-gram sizes
        std::vector<int32_t> view_plen, view_prefix;    // ... and forced prefixes (a sliver's prefix is ignored)
        std::vector<int32_t> view_automata;             // ... and automata
        std::vector<float> view_penalty;                // ... and repetition penalties
        for (int i = 0; i < n_rows; ++i) {
            const int v = view_of[req.source ? req.source[i] : i];
            if (v < 0) continue;
            where[i] = (int)view_src.size();
            view_src.push_back(v);
            if (req.sets) view_sets.push_back(req.sets[i]);
            if (req.ngram) view_ngram.push_back(req.ngram[i]);
            if (req.automata) view_automata.push_back(req.automata[i]);
            if (req.penalty) view_penalty.push_back(req.penalty[i]);
            if (req.prefix) {
                view_plen.push_back(req.prefix_len[i]);
                view_prefix.insert(view_prefix.end(), req.prefix + (size_t)i * req.prefix_ld, req.prefix + (size_t)(i + 1) * req.prefix_ld);
            }
        }
        // Every output the caller asked for: the caller's rows, the elements of a row, what a sliver's row
        // reads, and the recognised rows (a buffer of ours).  All hold 4-byte elements, moved as bytes: a fill value is
        // given as its bit pattern (0.f = 0, -1 = all ones).
        const size_t L = (size_t)e->cfg.max_len, nv = view_src.size();
        struct Out { void* dst; size_t per_row; uint32_t fill; std::vector<uint32_t> rows, sliver; };
        Out outs[] = {{out_ids, L, (uint32_t)e->cfg.pad_id, {}, {}},
                      {out_len, 1, 0u, {}, {}},
                      {req.out_logp, L, 0u, {}, {}},
                      {req.out_alt_ids, L * MOCR_ALTERNATIVES, 0xffffffffu, {}, {}},
                      {req.out_alt_logp, L * MOCR_ALTERNATIVES, 0u, {}, {}},
                      {req.out_pos, L * MOCR_POSITION_FIELDS, 0u, {}, {}},
                      {req.out_score, 1, 0xce6e6b28u /* -1e9f: beam search, a sliver's slots are empty */, {}, {}},
                      {req.out_state, 1, 0xffffffffu /* MOCR_STATE_NONE */, {}, {}}};
        for (Out& o : outs)
            if (o.dst) { o.rows.resize(nv * o.per_row); o.sliver.assign(o.per_row, o.fill); }
        auto rows_of = [&](int k) { return outs[k].dst ? outs[k].rows.data() : nullptr; };
        // prefix_ld 0 (validated: every length is 0 then) leaves no tokens to point at: the inner request carries no prefix,
        // so its two pointers stay both null or both set
        const bool pre = req.prefix && !view_prefix.empty();
        if (nv > 0) {
            Request inner = request_of(rows_of(2), rows_of(3), rows_of(4), req.sets ? view_sets.data() : nullptr,
                                       req.ngram ? view_ngram.data() : nullptr, rows_of(5), pre ? view_prefix.data() : nullptr,
                                       pre ? view_plen.data() : nullptr, pre ? req.prefix_ld : 0,
                                       req.source ? view_src.data() : nullptr, req.source ? (int32_t)views.size() : -1);
            inner.beam = req.beam; inner.out_score = reinterpret_cast<float*>(rows_of(6));      // (a sliver drops all K rows of its crop)
            inner.automata = req.automata ? view_automata.data() : nullptr; inner.out_state = reinterpret_cast<int32_t*>(rows_of(7));
            inner.penalty = req.penalty ? view_penalty.data() : nullptr;
            prepare_and_decode(e, srcs, views.data(), (int)nv, reinterpret_cast<int32_t*>(rows_of(0)), reinterpret_cast<int32_t*>(rows_of(1)), inner);
        }
        for (int i = 0; i < n_rows; ++i)
            for (Out& o : outs) {
                if (!o.dst) continue;
                const size_t bytes = o.per_row * sizeof(uint32_t);
                memcpy(static_cast<char*>(o.dst) + (size_t)i * bytes,
                       where[i] < 0 ? o.sliver.data() : o.rows.data() + (size_t)where[i] * o.per_row, bytes);
            }
    });
}

int mocr_recognize_regions_positions(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                     int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                     float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_regions, out_ids, out_len,
                             request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos));
}

int mocr_recognize_regions_prefix(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                  int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                  float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                  const int32_t* prefix_len, int32_t prefix_ld) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_regions, out_ids, out_len,
                             request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld));
}

int mocr_recognize_regions_shared(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                  int32_t n_regions, int32_t n_rows, const int32_t* source, int32_t* out_ids, int32_t* out_len,
                                  float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                  float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_rows, out_ids, out_len,
                             request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld, source,
                                        n_regions));
}

int mocr_recognize_regions_penalty(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                   int32_t n_regions, int32_t n_rows, const int32_t* source, int32_t* out_ids, int32_t* out_len,
                                   float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                   float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld,
                                   const int32_t* automata, int32_t* out_state, const float* penalty) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_rows, out_ids, out_len,
                             with_penalty(with_automata(request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len,
                                                                   prefix_ld, source, n_regions), automata, out_state), penalty));
}

int mocr_recognize_regions_automaton(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                     int32_t n_regions, int32_t n_rows, const int32_t* source, int32_t* out_ids, int32_t* out_len,
                                     float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                     float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld,
                                     const int32_t* automata, int32_t* out_state) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_rows, out_ids, out_len,
                             with_automata(request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram, out_pos, prefix, prefix_len, prefix_ld,
                                                      source, n_regions), automata, out_state));
}

int mocr_recognize_regions_norepeat(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                    int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                    float* out_alt_logp, const int32_t* sets, const int32_t* ngram) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_regions, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets, ngram));
}

int mocr_recognize_regions_constrained(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                       int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                       float* out_alt_logp, const int32_t* sets) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_regions, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp, sets));
}

int mocr_recognize_regions_alts(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                float* out_alt_logp) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_regions, out_ids, out_len, request_of(out_logp, out_alt_ids, out_alt_logp));
}

int mocr_recognize_regions_scored(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                  int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_regions, out_ids, out_len, request_of(out_logp));
}

int mocr_recognize_regions(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions, int32_t n_regions,
                           int32_t* out_ids, int32_t* out_len) {
    return recognize_regions(e, pages, n_pages, regions, n_regions, n_regions, out_ids, out_len, Request{});
}

// ---- beam search: the four source kinds.  A request of n crops is n K decode rows over n encodings - the shared-encodings
// request with source[c K + k] = c - plus the configuration and the score output; the checks come before any work.
// The *_beam_tokens twins add out_logp [n][K][max_len] = [rows][max_len] and one set handle per crop, expanded to its K rows;
// the *_beam_positions twins add out_pos [n][K][max_len][MOCR_POSITION_FIELDS] to those.
// The *_beam_automaton twins add one automaton handle per crop, expanded like the sets, and out_state [n][K] = [rows].
struct BeamCall { std::vector<int32_t> source, sets, automata; Request req; int rows = 0; };
static int beam_call(mocr_engine* e, const mocr_beam_config* beam, int32_t n, void* out_score, BeamCall& bc, void* out_logp = nullptr,
                     const int32_t* sets = nullptr, void* out_pos = nullptr, const int32_t* automata = nullptr, void* out_state = nullptr,
                     bool soft = false) {
    return guarded(e, [&] {
        if (!beam || beam->num_beams < 2 || beam->num_beams > MOCR_MAX_BEAMS) throw ArgError{"num_beams must be 2 .. MOCR_MAX_BEAMS (4)", MOCR_ERR_ARG};
        if (beam->early_stopping < 0 || beam->early_stopping > 2) throw ArgError{"early_stopping must be 0 (false), 1 (true) or 2 (never)", MOCR_ERR_ARG};
        if (beam->no_repeat_ngram_size < 0 || !std::isfinite(beam->length_penalty))
            throw ArgError{"no_repeat_ngram_size must be >= 0 and length_penalty finite", MOCR_ERR_ARG};
        if (n < 1) throw ArgError{"n must be positive", MOCR_ERR_ARG};
        if ((long long)n * beam->num_beams > e->cfg.max_batch) throw ArgError{"n * num_beams exceeds max_batch", MOCR_ERR_ARG};
        if (!out_score) throw ArgError{"null pointer", MOCR_ERR_ARG};
        const int K = beam->num_beams;
        bc.rows = n * K;
        bc.source.resize((size_t)bc.rows);
        for (int i = 0; i < bc.rows; ++i) bc.source[i] = i / K;
        bc.req.source = bc.source.data(); bc.req.n_images = n;
        bc.req.beam = beam; bc.req.out_score = static_cast<float*>(out_score);
        bc.req.out_logp = static_cast<float*>(out_logp);
        bc.req.out_pos = static_cast<float*>(out_pos);
        if (sets) {
            bc.sets.resize((size_t)bc.rows);
            for (int i = 0; i < bc.rows; ++i) bc.sets[i] = sets[i / K];
            bc.req.sets = bc.sets.data();        // (validate_request refuses an unknown handle)
        }
        if (automata) {
            bc.automata.resize((size_t)bc.rows);
            for (int i = 0; i < bc.rows; ++i) bc.automata[i] = automata[i / K];
            bc.req.automata = bc.automata.data();       // (likewise)
        }
        bc.req.out_state = static_cast<int32_t*>(out_state);
        bc.req.beam_soft = soft;
    });
}

int mocr_recognize_images_beam_tokens(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam, int32_t* out_ids,
                                      int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets)) return rc;
    return recognize_images(e, images, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_regions_beam_tokens(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                       int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                       float* out_score, float* out_logp, const int32_t* sets) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n_regions, out_score, bc, out_logp, sets)) return rc;
    return recognize_regions(e, pages, n_pages, regions, n_regions, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_gray_host_beam_tokens(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                         const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                         float* out_logp, const int32_t* sets) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets)) return rc;
    return recognize_gray_host(e, gray, bc.rows, max_len_override, out_ids, out_len, bc.req);
}

int mocr_recognize_device_beam_tokens(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                      void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, d_out_score, bc, d_out_logp, sets)) return rc;
    return recognize_device(e, d_gray, bc.rows, d_out_ids, d_out_len, bc.req);
}

int mocr_recognize_images_beam_positions(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam, int32_t* out_ids,
                                         int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets, float* out_pos) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets, out_pos)) return rc;
    return recognize_images(e, images, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_regions_beam_positions(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                          int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                          float* out_score, float* out_logp, const int32_t* sets, float* out_pos) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n_regions, out_score, bc, out_logp, sets, out_pos)) return rc;
    return recognize_regions(e, pages, n_pages, regions, n_regions, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_gray_host_beam_positions(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                            const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                            float* out_logp, const int32_t* sets, float* out_pos) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets, out_pos)) return rc;
    return recognize_gray_host(e, gray, bc.rows, max_len_override, out_ids, out_len, bc.req);
}

int mocr_recognize_device_beam_positions(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                         void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets, void* d_out_pos) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, d_out_score, bc, d_out_logp, sets, d_out_pos)) return rc;
    return recognize_device(e, d_gray, bc.rows, d_out_ids, d_out_len, bc.req);
}

int mocr_recognize_images_beam_automaton(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam, int32_t* out_ids,
                                         int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                         const int32_t* automata, int32_t* out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets, out_pos, automata, out_state)) return rc;
    return recognize_images(e, images, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_regions_beam_automaton(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                          int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                          float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                          const int32_t* automata, int32_t* out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n_regions, out_score, bc, out_logp, sets, out_pos, automata, out_state)) return rc;
    return recognize_regions(e, pages, n_pages, regions, n_regions, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_gray_host_beam_automaton(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                            const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                            float* out_logp, const int32_t* sets, float* out_pos, const int32_t* automata,
                                            int32_t* out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets, out_pos, automata, out_state)) return rc;
    return recognize_gray_host(e, gray, bc.rows, max_len_override, out_ids, out_len, bc.req);
}

int mocr_recognize_device_beam_automaton(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                         void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets, void* d_out_pos,
                                         const int32_t* automata, void* d_out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, d_out_score, bc, d_out_logp, sets, d_out_pos, automata, d_out_state)) return rc;
    return recognize_device(e, d_gray, bc.rows, d_out_ids, d_out_len, bc.req);
}

// The *_beam_soft twins: the *_beam_automaton calls with soft handles allowed (without one they ARE those calls).
int mocr_recognize_images_beam_soft(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam, int32_t* out_ids,
                                    int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                    const int32_t* automata, int32_t* out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets, out_pos, automata, out_state, true)) return rc;
    return recognize_images(e, images, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_regions_beam_soft(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                     int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                     float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                     const int32_t* automata, int32_t* out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n_regions, out_score, bc, out_logp, sets, out_pos, automata, out_state, true)) return rc;
    return recognize_regions(e, pages, n_pages, regions, n_regions, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_gray_host_beam_soft(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                       const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                       float* out_logp, const int32_t* sets, float* out_pos, const int32_t* automata,
                                       int32_t* out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc, out_logp, sets, out_pos, automata, out_state, true)) return rc;
    return recognize_gray_host(e, gray, bc.rows, max_len_override, out_ids, out_len, bc.req);
}

int mocr_recognize_device_beam_soft(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                    void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets, void* d_out_pos,
                                    const int32_t* automata, void* d_out_state) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, d_out_score, bc, d_out_logp, sets, d_out_pos, automata, d_out_state, true)) return rc;
    return recognize_device(e, d_gray, bc.rows, d_out_ids, d_out_len, bc.req);
}

int mocr_recognize_images_beam(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam, int32_t* out_ids,
                               int32_t* out_len, float* out_score) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc)) return rc;
    return recognize_images(e, images, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_regions_beam(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions, int32_t n_regions,
                                const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n_regions, out_score, bc)) return rc;
    return recognize_regions(e, pages, n_pages, regions, n_regions, bc.rows, out_ids, out_len, bc.req);
}

int mocr_recognize_gray_host_beam(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, const mocr_beam_config* beam,
                                  int32_t* out_ids, int32_t* out_len, float* out_score) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, out_score, bc)) return rc;
    return recognize_gray_host(e, gray, bc.rows, max_len_override, out_ids, out_len, bc.req);
}

int mocr_recognize_device_beam(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids, void* d_out_len,
                               void* d_out_score) {
    BeamCall bc;
    if (const int rc = beam_call(e, beam, n, d_out_score, bc)) return rc;
    return recognize_device(e, d_gray, bc.rows, d_out_ids, d_out_len, bc.req);
}

int mocr_set_generate_max_length(mocr_engine* e, int32_t max_len) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (max_len < 2 || max_len > e->cfg.max_len) throw ArgError{"generate max_length must be in [2, max_len]", MOCR_ERR_ARG};
        e->gen_max_len = max_len;
    });
}

int mocr_ln_fold_state(mocr_engine* e, float* noise_ratio) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    if (noise_ratio) *noise_ratio = e->fold_ratio;
    if (e->cfg.dtype != MOCR_BF16 || (e->cfg.flags & MOCR_FLAG_NO_LN_FOLD)) return 0;
    return (e->fold_ok || (e->cfg.flags & MOCR_FLAG_FORCE_LN_FOLD)) ? 1 : 0;
}

int64_t mocr_decode_slot_steps(mocr_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return e->n_slot_steps;
}

int64_t mocr_encoded_crops(mocr_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return e->n_encoded;
}

int64_t mocr_compaction_count(mocr_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return e->n_compactions;
}

int mocr_graph_count(mocr_engine* e) {
    if (!e) return MOCR_ERR_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return (int)e->graphs.size();
}

int mocr_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes) {
    if (!free_bytes || !total_bytes) return MOCR_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return MOCR_ERR_HIP;
    size_t f = 0, t = 0;
    if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess) return MOCR_ERR_HIP;
    *free_bytes = (int64_t)f; *total_bytes = (int64_t)t;
    return MOCR_OK;
}

int mocr_encode(mocr_engine* e, const void* d_gray, int32_t n, float* h_out) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        require_ready(e, n);
        if (!d_gray || !h_out) throw ArgError{"null pointer", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->bind(0);
        const uint8_t* g = reinterpret_cast<const uint8_t*>(d_gray);
        dispatch(e, [&](auto tag) { run_encoder<decltype(tag)>(e, g, n); });
        const size_t count = (size_t)n * e->S * e->D;
        if (e->cfg.dtype == MOCR_F32) {
            HIPCHECK(hipMemcpyAsync(h_out, e->ENC, count * 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
        } else {
            std::vector<uint16_t> tmp(count);
            HIPCHECK(hipMemcpyAsync(tmp.data(), e->ENC, count * 2, hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
            for (size_t i = 0; i < count; ++i) {
                const uint32_t u = (uint32_t)tmp[i] << 16;
                memcpy(&h_out[i], &u, 4);
            }
        }
    });
}

int mocr_decode_logits(mocr_engine* e, const void* d_gray, int32_t n, const int32_t* forced_ids, int32_t T, float* h_logits) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        require_ready(e, n);
        if (!d_gray || !forced_ids || !h_logits || T < 1 || T >= e->cfg.max_len) throw ArgError{"bad argument", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->bind(0);
        const size_t fcount = (size_t)n * T, lcount = (size_t)n * T * e->V;
        if (fcount > e->forced_cap) { e->forced = e->dalloc<int>(fcount); e->forced_cap = fcount; }
        if (lcount > e->logits_cap) { e->logits_dbg = e->dalloc<float>(lcount); e->logits_cap = lcount; }
        e->unbind(0);
        HIPCHECK(hipMemcpyAsync(e->forced, forced_ids, fcount * sizeof(int), hipMemcpyHostToDevice, e->stream));
        const uint8_t* g = reinterpret_cast<const uint8_t*>(d_gray);
        dispatch(e, [&](auto tag) {
            using T_ = decltype(tag);
            run_encoder<T_>(e, g, n);
            if (!e->use_latent(n)) run_cross_kv<T_>(e, n);
            else if (e->fp8attn) quantize_enc(e, n);
            run_decode_forced<T_>(e, n, e->forced, T, e->logits_dbg);
        });
        HIPCHECK(hipMemcpyAsync(h_logits, e->logits_dbg, lcount * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
    });
}

int mocr_op_gemm(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, void* d_out, const float* d_resid,
                 int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t tile, int32_t split_k) {
    return op_hook(e, [&] {
        if (epilogue == EPI_PATCH || epilogue == EPI_ARGMAX || epilogue == EPI_ARGMAX_LSE || epilogue == EPI_TOPK)
            throw ArgError{"EPI_PATCH / EPI_ARGMAX are not exposed through mocr_op_gemm (EPI_ARGMAX: mocr_op_gemm_argmax)", MOCR_ERR_ARG};
        GemmCall c = gemm_call("op_gemm", dA, K, dW, d_bias, d_out, N, M, N, K, epilogue, tile);
        c.resid = d_resid; c.split = split_k; c.slab_stride = (long long)M * N;
        if (e->cfg.dtype == MOCR_BF16) gemm<bf16_t>(e, c); else gemm<float>(e, c);
    });
}

int mocr_op_gemm_ln(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, void* d_out, const float* d_resid,
                    int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t tile, float* d_part, const float* d_csum, void* d_xb) {
    return op_hook(e, [&] {
        if (e->cfg.dtype != MOCR_BF16) throw ArgError{"mocr_op_gemm_ln: bf16 engines only", MOCR_ERR_UNSUPPORTED};
        LnFold f{d_part, d_csum, d_xb};
        GemmCall c = gemm_call("op_gemm_ln", dA, K, dW, d_bias, d_out, N, M, N, K, epilogue, tile);
        c.resid = d_resid; c.lnf = &f;
        gemm<bf16_t>(e, c);
    });
}

int mocr_op_ln_prep(mocr_engine* e, const float* d_x, void* d_xb, float* d_part, int32_t M) {
    return op_hook(e, [&] {
        if (e->D != 768) throw ArgError{"mocr_op_ln_prep: hidden size 768 only", MOCR_ERR_UNSUPPORTED};
        hipLaunchKernelGGL((ln_prep_kernel<768>), dim3((M + 3) / 4), dim3(256), 0, e->stream, d_x, reinterpret_cast<bf16_t*>(d_xb), d_part, M);
        HIPCHECK(hipGetLastError());
    });
}

int mocr_op_layernorm(mocr_engine* e, const float* d_x, const float* d_gamma, const float* d_beta, void* d_out, int32_t M) {
    return op_hook(e, [&] {
        dispatch(e, [&](auto tag) { layernorm<decltype(tag)>(e, d_x, d_gamma, d_beta, d_out, M); });
    });
}

int mocr_op_enc_attention(mocr_engine* e, const void* d_qkv, void* d_ctx, int32_t n, int32_t impl) {
    return op_hook(e, [&] {
        dispatch(e, [&](auto tag) {
            using T_ = decltype(tag);
            enc_attention<T_>(e, d_qkv, d_ctx, n, impl, enc_attn_ysplit<T_>(e, n, impl));
        });
    });
}

int mocr_op_embed(mocr_engine* e, const void* d_gray, int32_t n, int32_t tile, void* d_patches, float* d_x) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        require_ready(e, n);
        if (!d_gray || !d_patches || !d_x) throw ArgError{"mocr_op_embed: null pointer", MOCR_ERR_ARG};
        if (tile != 0 && tile != 64 && tile != 128) throw ArgError{"mocr_op_embed: tile must be 0 (the encoder's choice), 64 or 128", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->bind(0);
        const uint8_t* g = reinterpret_cast<const uint8_t*>(d_gray);
        dispatch(e, [&](auto tag) { encoder_front<decltype(tag)>(e, g, n, d_patches, d_x, tile); });
        HIPCHECK(hipStreamSynchronize(e->stream));
    });
}

int mocr_op_layernorm_slab(mocr_engine* e, float* d_x, const float* d_slabs, int32_t nslab, int64_t slab_stride, const float* d_bias,
                           const float* d_gamma, const float* d_beta, void* d_out, int32_t M) {
    return op_hook(e, [&] {
        if (e->D != 768) throw ArgError{"mocr_op_layernorm_slab: hidden size 768 only", MOCR_ERR_UNSUPPORTED};
        if (!d_x || !d_slabs || !d_bias || !d_gamma || !d_beta || !d_out || nslab < 1 || M < 1 || slab_stride < (int64_t)M * e->D ||
            (slab_stride & 3))
            throw ArgError{"mocr_op_layernorm_slab: bad argument", MOCR_ERR_ARG};
        dispatch(e, [&](auto tag) {
            layernorm_slab<decltype(tag)>(e, d_x, d_slabs, nslab, (long long)slab_stride, d_bias, d_gamma, d_beta, d_out, M);
        });
    });
}

int mocr_encoder_plan(mocr_engine* e, int32_t n, int32_t out[10]) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        require_ready(e, n);
        if (!out) throw ArgError{"mocr_encoder_plan: null pointer", MOCR_ERR_ARG};
        EncPlan pl{};
        dispatch(e, [&](auto tag) { pl = encoder_plan<decltype(tag)>(e, n); });
        const int32_t v[10] = {pl.embed_tile, pl.tq, pl.to, pl.t1, pl.t2, pl.split_o, pl.split_2, pl.fold ? 1 : 0, pl.ysplit, pl.impl};
        memcpy(out, v, sizeof(v));
    });
}

int mocr_encoder_groups(mocr_engine* e, int32_t n, int32_t out[2]) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        require_ready(e, n);
        if (!out) throw ArgError{"mocr_encoder_groups: null pointer", MOCR_ERR_ARG};
        EncPlan pl{};
        dispatch(e, [&](auto tag) { pl = encoder_plan<decltype(tag)>(e, n); });
        out[0] = pl.gq; out[1] = pl.g1;
    });
}

int mocr_decode_plan(mocr_engine* e, int32_t rows, int32_t regime_rows, int32_t out[MOCR_DECODE_PLAN_FIELDS]) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!e->committed) throw ArgError{"mocr_decode_plan: weights not committed", MOCR_ERR_ARG};
        if (!out || rows < 1 || regime_rows < 0) throw ArgError{"mocr_decode_plan: bad argument", MOCR_ERR_ARG};
        DecPlan pl{};
        {
            RegimeScope rs(e, regime_rows);
            dispatch(e, [&](auto tag) { pl = decode_plan<decltype(tag)>(e, rows); });
        }
        int32_t v[MOCR_DECODE_PLAN_FIELDS] = {pl.path, pl.regime_tile, pl.launch_tile};
        for (int i = 0; i < 5; ++i) { v[3 + 3 * i] = pl.g[i].split; v[4 + 3 * i] = pl.g[i].ring; v[5 + 3 * i] = pl.g[i].epi; }
        const int32_t tail[7] = {pl.qkv_tile_gemm, pl.qqt, pl.qqt_bm, pl.qt_tile, pl.attn_nt, pl.chunk, pl.graph_rows};
        memcpy(v + 18, tail, sizeof(tail));
        static_assert(MOCR_DECODE_PLAN_FIELDS == 25, "mocr_decode_plan's layout");
        memcpy(out, v, sizeof(v));
    });
}

int mocr_op_gemm_args(mocr_engine* e, const mocr_gemm_args* a) {
    return op_hook(e, [&] {
        if (!a || a->struct_size != (int32_t)sizeof(mocr_gemm_args)) throw ArgError{"mocr_op_gemm_args: bad struct_size", MOCR_ERR_ARG};
        const int epi = a->epilogue;
        if (epi == EPI_PATCH || epi == EPI_ARGMAX || epi == EPI_ARGMAX_LSE || epi == EPI_TOPK)
            throw ArgError{"EPI_PATCH / EPI_ARGMAX are not exposed through mocr_op_gemm_args (EPI_ARGMAX: mocr_op_gemm_argmax)", MOCR_ERR_ARG};
        const int esz = e->cfg.dtype == MOCR_BF16 ? 2 : 4;
        const int lda = a->lda ? a->lda : a->K, ldo = a->ldo ? a->ldo : a->N;
        if (!a->A || !a->W || !a->out || a->M < 1 || a->N < 1 || a->K < 1 || a->split_k < 1 || a->group_n < 0 ||
            (epi != EPI_SLAB && !a->bias) || (epi == EPI_BIAS_RESID && !a->resid))
            throw ArgError{"mocr_op_gemm_args: bad argument", MOCR_ERR_ARG};
        if (!tile_is(a->tile, GemmKind::Tile)) throw ArgError{"mocr_op_gemm_args: the tile GEMM only (tile 64 or 128)", MOCR_ERR_ARG};
        // rows are fetched and stored in 16-byte pieces
        if (lda < a->K || (lda * esz) % 16 || ldo < a->N || ldo % 4)
            throw ArgError{"mocr_op_gemm_args: lda >= K and ldo >= N, rows 16-byte aligned", MOCR_ERR_ARG};
        const long long dense = (long long)(a->M - 1) * ldo + a->N;       // elements one slab spans
        const long long slab_stride = a->slab_stride ? a->slab_stride : (long long)a->M * ldo;
        if (epi == EPI_SLAB && (slab_stride < dense || (slab_stride & 3)))
            throw ArgError{"mocr_op_gemm_args: slab_stride must hold a slab and be a multiple of 4", MOCR_ERR_ARG};
        GemmCall c = gemm_call("op_gemm", a->A, lda, a->W, a->bias, a->out, ldo, a->M, a->N, a->K, epi, a->tile);
        c.resid = a->resid; c.split = a->split_k; c.slab_stride = slab_stride; c.group_n = a->group_n;
        if (e->cfg.dtype == MOCR_BF16) gemm<bf16_t>(e, c); else gemm<float>(e, c);
    });
}

int mocr_last_tile_launch(mocr_engine* e, int32_t out[4]) {
    return guarded(e, [&] {
        if (!out) throw ArgError{"mocr_last_tile_launch: null pointer", MOCR_ERR_ARG};
        const int32_t v[4] = {g_last_tile.bm, g_last_tile.ring, g_last_tile.blocks, g_last_tile.split};
        memcpy(out, v, sizeof(v));
    });
}

int mocr_op_gemm_pers(mocr_engine* e, const mocr_gemm_pers_args* a) {
    return op_hook(e, [&] {
        if (!a || a->struct_size != (int32_t)sizeof(mocr_gemm_pers_args)) throw ArgError{"mocr_op_gemm_pers: bad struct_size", MOCR_ERR_ARG};
        if (e->cfg.dtype != MOCR_BF16) throw ArgError{"mocr_op_gemm_pers: bf16 engines only", MOCR_ERR_UNSUPPORTED};
        const int epi = a->epilogue;
        if (epi != EPI_BIAS && epi != EPI_BIAS_GELU && epi != EPI_BIAS_RESID)
            throw ArgError{"mocr_op_gemm_pers: epilogue 1 (bias), 2 (bias + GELU) or 3 (bias + residual)", MOCR_ERR_ARG};
        if (!a->A || !a->W || !a->bias || !a->out || a->M < 1 || a->N < 1 || a->K < 1 || a->group_n < 0 || (epi == EPI_BIAS_RESID && !a->resid) ||
            ((a->csum || a->xb) && !a->ln_part))
            throw ArgError{"mocr_op_gemm_pers: bad argument", MOCR_ERR_ARG};
        if (a->tile < TILE_PERSISTENT) throw ArgError{"mocr_op_gemm_pers: the persistent kernel only (tile codes from 4096)", MOCR_ERR_ARG};
        // the GemmCall run_encoder builds for a layer GEMM: dense rows, the residual, the column groups, the fold operands
        const LnFold f{a->ln_part, a->csum, a->xb};
        GemmCall c = gemm_call("op_gemm_pers", a->A, a->K, a->W, a->bias, a->out, a->N, a->M, a->N, a->K, epi, a->tile);
        c.resid = a->resid; c.group_n = a->group_n;
        if (a->ln_part) c.lnf = &f;
        gemm<bf16_t>(e, c);
    });
}

int mocr_last_pers_launch(mocr_engine* e, int32_t out[4]) {
    return guarded(e, [&] {
        if (!out) throw ArgError{"mocr_last_pers_launch: null pointer", MOCR_ERR_ARG};
        const int32_t v[4] = {g_last_pers.blocks, g_last_pers.strips, g_last_pers.tiles, g_last_pers.group_n};
        memcpy(out, v, sizeof(v));
    });
}

int mocr_op_latent_attention(mocr_engine* e, const void* d_qt, const void* d_x, void* d_out, int32_t n, int32_t len,
                             int64_t x_batch_stride) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->bind(0);
        if (e->cfg.dtype != MOCR_BF16 || !d_qt || !d_x || !d_out || n < 1 || len < 1) throw ArgError{"bad argument", MOCR_ERR_ARG};
        LatentParams p{};
        p.qt = reinterpret_cast<const bf16_t*>(d_qt); p.x = reinterpret_cast<const bf16_t*>(d_x);
        p.out = reinterpret_cast<bf16_t*>(d_out); p.x_batch_stride = x_batch_stride; p.fixed_len = len; p.heads = e->H;
        p.ablate = env_int("MOCR_LAT_ABLATE", 0); p.rows = n;
        static unsigned long long* dbg = nullptr;
        if (env_int("MOCR_LAT_STAMP", 0)) { if (!dbg) dbg = e->dalloc<unsigned long long>(8 + 512); p.dbg = dbg; }
        ProfScope ps(e, "op_latent", 0, (double)n * len * 1536);
        launch_latent(e, false, p);
        HIPCHECK(hipStreamSynchronize(e->stream));
        if (p.dbg) {
            unsigned long long h[40];
            HIPCHECK(hipMemcpy(h, p.dbg, sizeof(h), hipMemcpyDeviceToHost));
            if (env_int("MOCR_LAT_DUMP", 0)) {
                std::vector<float> f(1024);
                HIPCHECK(hipMemcpy(f.data(), p.dbg + 8, 1024 * 4, hipMemcpyDeviceToHost));
                FILE* fp = fopen("gpurun_out/lat_dump.bin", "wb");
                if (fp) { fwrite(f.data(), 4, 1024, fp); fclose(fp); }
            }
            for (int w = 0; w < 4; ++w)
                fprintf(stderr, "[lat stamps, cycles, block 0 wave %d] wait+issue %llu  S %llu  exchange %llu  softmax %llu  PX %llu  loop/Qt %llu  rowend-b1 %llu  stage-b2 %llu  store %llu\n",
                        w, h[10 * w], h[10 * w + 1], h[10 * w + 2], h[10 * w + 3], h[10 * w + 4], h[10 * w + 5], h[10 * w + 6], h[10 * w + 7], h[10 * w + 8]);
        }
    });
}

int mocr_op_quant_fp8(mocr_engine* e, const void* d_x, void* d_x8, int64_t n_elems, float inv_sx) {
    return op_hook(e, [&] {
        if (!d_x || !d_x8 || n_elems < 16 || n_elems % 16) throw ArgError{"bad argument (n_elems must be a positive multiple of 16)", MOCR_ERR_ARG};
        const long long n16 = n_elems / 16;
        hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, e->stream,
                           reinterpret_cast<const bf16_t*>(d_x), reinterpret_cast<uint8_t*>(d_x8), n16, inv_sx);
        HIPCHECK(hipGetLastError());
    });
}

int mocr_op_latent_attention_fp8(mocr_engine* e, const void* d_qt, const void* d_x8, void* d_out, int32_t n, int32_t len,
                                 int64_t x_batch_stride_bytes, float sx) {
    return op_hook(e, [&] {
        if (e->cfg.dtype != MOCR_BF16 || !d_qt || !d_x8 || !d_out || n < 1 || len < 1 || !(sx > 0.f)) throw ArgError{"bad argument", MOCR_ERR_ARG};
        Latent8Params p{};
        p.qt = reinterpret_cast<const bf16_t*>(d_qt); p.x8 = reinterpret_cast<const uint8_t*>(d_x8);
        p.out = reinterpret_cast<bf16_t*>(d_out); p.x_batch_stride = x_batch_stride_bytes; p.fixed_len = len; p.heads = e->H;
        p.rows = n; p.sx = sx;
        ProfScope ps(e, "op_latent8", 0, (double)n * len * 768);
        launch_latent8(e, false, p);
    });
}

int mocr_op_qqt(mocr_engine* e, const void* d_x, const void* d_wq, const float* d_bq, const void* d_wkT, void* d_qt, int32_t n) {
    return op_hook(e, [&] {
        if (e->cfg.dtype != MOCR_BF16 || !d_x || !d_wq || !d_bq || !d_wkT || !d_qt || n < 1) throw ArgError{"bad argument", MOCR_ERR_ARG};
        QqtParams q{};
        q.x = reinterpret_cast<const bf16_t*>(d_x); q.wq = reinterpret_cast<const bf16_t*>(d_wq); q.bq = d_bq;
        q.wkT = reinterpret_cast<const bf16_t*>(d_wkT); q.qt = reinterpret_cast<bf16_t*>(d_qt);
        ProfScope ps(e, "op_qqt", 4.0 * n * 768 * 768, 0);
        launch_qqt(e, q, n, n);
    });
}

int mocr_op_dec_attn(mocr_engine* e, int32_t self, const float* d_slabs, int32_t nslab, const float* d_bias, void* d_k, void* d_v,
                     int32_t layer, const int32_t* d_step, const int32_t* d_rowmap, void* d_ctx, int32_t n, int32_t approx_len,
                     int32_t nt) {
    return op_hook(e, [&] {
        if (!e->committed || !d_slabs || !d_bias || !d_k || !d_ctx || n < 1 || nslab < 1 || nt < -1 || nt > 1 || e->D != 768 ||
            (self && (!d_v || !d_step || approx_len < 1 || approx_len > e->cfg.max_len)) ||
            (!self && (layer < 0 || layer >= e->cfg.dec_layers)))
            throw ArgError{"mocr_op_dec_attn: bad argument", MOCR_ERR_ARG};
        dispatch(e, [&](auto tag) {
            using T_ = decltype(tag);
            if (self) {
                DecAttnParams p = dec_attn_block<T_, true>(e, d_slabs, n, nslab, d_bias, d_k, d_v, 0, d_step, d_rowmap, d_ctx, n);
                if (nt >= 0) p.nt = nt;
                launch_dec_attn<T_, true>(e, p, n, approx_len);
            } else {
                DecAttnParams p = dec_attn_block<T_, false>(e, d_slabs, n, nslab, d_bias, d_k, nullptr, layer, nullptr, d_rowmap, d_ctx, n);
                if (nt >= 0) p.nt = nt;
                launch_dec_attn<T_, false>(e, p, n, e->S);
            }
        });
    });
}

int mocr_op_dec_add_ln(mocr_engine* e, const float* d_slabs, int32_t nslab, const float* d_bias, const float* d_resid,
                       const float* d_gamma, const float* d_beta, int32_t gelu, float* d_out_f32, void* d_out_t, int32_t rows,
                       void* d_cache, int32_t cache_fp8, float inv_sx, const int32_t* d_step, const int32_t* d_rowmap) {
    return op_hook(e, [&] {
        if (!e->committed || !d_slabs || !d_bias || !d_gamma || !d_beta || !d_out_t || rows < 1 || nslab < 1 || e->D != 768 ||
            (d_cache && !d_step))
            throw ArgError{"mocr_op_dec_add_ln: bad argument", MOCR_ERR_ARG};
        DecAddLnArgs a{};
        a.slabs = d_slabs; a.nslab = nslab; a.slab_stride = (long long)rows * e->D;
        a.bias = d_bias; a.resid = d_resid; a.g = d_gamma; a.b = d_beta; a.out_f32 = d_out_f32; a.out_t = d_out_t; a.rows = rows;
        a.gelu = gelu != 0;
        a.cstride = (long long)e->cfg.max_len * e->D;
        a.step = d_step; a.rowmap = d_rowmap;
        if (d_cache && cache_fp8) { a.cache8 = reinterpret_cast<uint8_t*>(d_cache); a.inv8 = inv_sx; }
        else a.cache = d_cache;
        dispatch(e, [&](auto tag) { launch_dec_add_ln<decltype(tag)>(e, a); });
    });
}

int mocr_op_dec_bias_gelu(mocr_engine* e, const float* d_slabs, int32_t nslab, const float* d_bias, void* d_out, int32_t rows,
                          int32_t N) {
    return op_hook(e, [&] {
        if (!d_slabs || !d_bias || !d_out || rows < 1 || nslab < 1 || N < 4 || N % 4)
            throw ArgError{"mocr_op_dec_bias_gelu: bad argument", MOCR_ERR_ARG};
        dispatch(e, [&](auto tag) { launch_dec_bias_gelu<decltype(tag)>(e, d_slabs, nslab, (long long)rows * N, d_bias, d_out, rows, N); });
    });
}

int mocr_op_attn_positions(mocr_engine* e, const void* d_q, const void* d_k, const int32_t* d_len, int32_t rows, int32_t T, float* d_out_pos,
                           float* d_out_map) {
    return mocr_op_attn_positions_gathered(e, d_q, d_k, d_len, rows, T, d_out_pos, d_out_map, nullptr, 0, 0);
}

int mocr_op_attn_positions_gathered(mocr_engine* e, const void* d_q, const void* d_k, const int32_t* d_len, int32_t rows, int32_t T,
                                    float* d_out_pos, float* d_out_map, const uint8_t* d_trail, int32_t trail_ld, int32_t K) {
    return op_hook(e, [&] {
        if (!e->committed || !d_q || !d_k || !d_len || !d_out_pos || rows < 1 || T < 1)
            throw ArgError{"mocr_op_attn_positions: bad argument", MOCR_ERR_ARG};
        // positions at and behind d_len read 0: the kernel writes the computed ones only
        HIPCHECK(hipMemsetAsync(d_out_pos, 0, (size_t)rows * T * MOCR_POSITION_FIELDS * sizeof(float), e->stream));
        if (d_out_map) HIPCHECK(hipMemsetAsync(d_out_map, 0, (size_t)rows * T * POS_KEYS * sizeof(float), e->stream));
        PosParams p{};
        p.q = d_q; p.q_row_stride = (long long)T * e->D;
        p.k = d_k; p.k_row_stride = (long long)e->S * e->D;
        p.len = d_len; p.len_bias = 0; p.T = T;
        p.out_pos = d_out_pos; p.pos_row_stride = (long long)T * MOCR_POSITION_FIELDS;
        p.out_map = d_out_map;
        if (d_trail) { p.trail = d_trail; p.trail_ld = trail_ld; p.K = K; }      // (launch_attn_positions checks the three)
        if (e->cfg.dtype == MOCR_BF16) launch_attn_positions<bf16_t>(e, p, rows); else launch_attn_positions<float>(e, p, rows);
    });
}

// The expansion of shared encodings as start_batch runs it, on the caller's buffer: its first n_src rows are staged in the
// lane's CTX, then row r of it becomes staged row d_src_of_row[r].
int mocr_op_enc_expand(mocr_engine* e, void* d_enc, const int32_t* d_src_of_row, int32_t n_src, int32_t n_rows) {
    return op_hook(e, [&] {
        const size_t row_bytes = (size_t)e->S * e->D * e->esz;
        if (!d_enc || !d_src_of_row || n_src < 1 || n_rows < 1 || n_src > e->cfg.max_batch || n_rows > e->cfg.max_batch ||
            (size_t)n_src * row_bytes > e->ctx_cap)
            throw ArgError{"mocr_op_enc_expand: bad argument", MOCR_ERR_ARG};
        std::vector<int32_t> h((size_t)n_rows);
        HIPCHECK(hipMemcpy(h.data(), d_src_of_row, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t v : h)
            if (v < 0 || v >= n_src) throw ArgError{"mocr_op_enc_expand: source index outside [0, n_src)", MOCR_ERR_ARG};
        HIPCHECK(hipMemcpyAsync(e->CTX, d_enc, (size_t)n_src * row_bytes, hipMemcpyDeviceToDevice, e->stream));
        launch_enc_expand(e, e->CTX, d_enc, d_src_of_row, n_src, n_rows);
    });
}

int mocr_op_ngram_init(mocr_engine* e, uint32_t* d_row_mask, const uint32_t* d_base_mask, const int32_t* d_base_set_of_row,
                       const int32_t* d_ngram_of_row, int32_t rows) {
    return op_hook(e, [&] {
        if (!e->committed || !d_row_mask || !d_base_mask || !d_base_set_of_row || !d_ngram_of_row || rows < 1 || e->V % 32)
            throw ArgError{"mocr_op_ngram_init: bad argument", MOCR_ERR_ARG};
        launch_ngram_init(e, d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, rows);
    });
}

// What the mocr_op_dec_token* symbols bring beside mocr_token_args, by feature, in the manner of LmHead (a group left out: null)
struct TokenOp {
    struct Scored { const float* cand_sum; float* scores; } scored{};
    struct Alts { const float* top_val; const int32_t* top_idx; int32_t* alt_ids; float* alt_logp; } alts{};
    struct Sets { const uint32_t* tok_mask; const int32_t* set_of_row; } sets{};
    struct Ngram { uint32_t* row_mask; const uint32_t* base_mask; const int32_t* base_set_of_row; const int32_t* ngram_of_row; } ngram{};
    struct Prefix { const int32_t* prefix; const int32_t* prefix_len; int32_t prefix_ld; const float* tgt_val; } prefix{};
    DecPenAutomata aut{};           // the automaton tables and the rows' states {{{six}, edge_weight, default_next}, {seen_mask, penalty_of_row}}
};

// The token kernel on the caller's buffers: the mocr_op_dec_token* symbols are this with some of the groups left out.
static int op_dec_token(mocr_engine* e, const mocr_token_args* a, const TokenOp& o = {}) {
    return op_hook(e, [&] {
        const auto [d_cand_sum, d_scores] = o.scored;
        const auto [d_top_val, d_top_idx, d_alt_ids, d_alt_logp] = o.alts;
        const auto [d_tok_mask, d_set_of_row] = o.sets;
        const auto [d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row] = o.ngram;
        const auto [d_prefix, d_prefix_len, prefix_ld, d_tgt_val] = o.prefix;
        const auto d_edge_begin = o.aut.edge_begin, d_edge_token = o.aut.edge_token, d_edge_next = o.aut.edge_next,
                   d_aut_base_of_row = o.aut.base_of_row, d_default_next = o.aut.default_next;
        const auto d_accepting = o.aut.accepting;
        const auto d_aut_state = o.aut.state;
        const auto d_edge_weight = o.aut.edge_weight, d_penalty_of_row = o.aut.pen.penalty_of_row;
        const auto d_seen_mask = o.aut.pen.seen_mask;
        if (!a || a->struct_size != (int32_t)sizeof(mocr_token_args)) throw ArgError{"mocr_op_dec_token: bad struct_size", MOCR_ERR_ARG};
        const bool first = a->first != 0;
        if (!e->committed || a->n < 1 || !a->ids || !a->step || !a->finished || !a->len || !a->n_unfinished || !a->rowmap ||
            !a->x_f32 || !a->x_t || a->ids_ld < 1 || a->max_len < 2 || a->max_len > e->cfg.max_len || e->D != 768 || e->V != 6144 ||
            (!first && a->ncand > 0 && (!a->cand_val || !a->cand_idx)) ||
            (!first && a->ncand <= 0 && (!a->slabs || a->nslab < 1)) || (a->forced && a->forced_T < 1) ||
            (d_scores && (first || a->forced || (a->ncand > 0 && !d_cand_sum))) ||
            ((d_alt_ids == nullptr) != (d_alt_logp == nullptr)) || (d_alt_ids && (!d_scores || (a->ncand > 0 && (!d_top_val || !d_top_idx)))) ||
            ((d_tok_mask == nullptr) != (d_set_of_row == nullptr)) || (d_tok_mask && (first || a->forced)) ||
            ((d_row_mask == nullptr) != (d_base_mask == nullptr)) || ((d_row_mask == nullptr) != (d_base_set_of_row == nullptr)) ||
            ((d_row_mask == nullptr) != (d_ngram_of_row == nullptr)) || (d_row_mask && !d_tok_mask) ||
            ((d_prefix == nullptr) != (d_prefix_len == nullptr)) ||
            (d_prefix && (!d_scores || !d_tok_mask || prefix_ld < 1 || (a->ncand > 0 && !d_tgt_val))) ||
            ((d_aut_state == nullptr) != (d_edge_begin == nullptr)) || ((d_aut_state == nullptr) != (d_edge_token == nullptr)) ||
            ((d_aut_state == nullptr) != (d_edge_next == nullptr)) || ((d_aut_state == nullptr) != (d_accepting == nullptr)) ||
            ((d_aut_state == nullptr) != (d_aut_base_of_row == nullptr)) || (d_aut_state && !d_row_mask) ||
            ((d_edge_weight == nullptr) != (d_default_next == nullptr)) || (d_edge_weight && !d_aut_state) ||
            // (the PEN form is a SOFT one: a penalty comes with the per-row masks, on the 6144-token vocabulary, and an
            // automaton beside it is given with its weights and default edges)
            ((d_seen_mask == nullptr) != (d_penalty_of_row == nullptr)) ||
            (d_seen_mask && (!d_row_mask || e->V != 6144 || first || (d_aut_state && !d_edge_weight))))
            throw ArgError{"mocr_op_dec_token: bad argument", MOCR_ERR_ARG};
        DecState st{};
        st.n_real = a->n_real;
        st.ids = a->ids; st.step = a->step; st.finished = a->finished; st.len = a->len; st.n_unfinished = a->n_unfinished;
        st.forced = a->forced; st.forced_T = a->forced_T; st.logits_out = nullptr;
        st.ids_ld = a->ids_ld; st.max_len = a->max_len;
        st.start_id = e->cfg.start_id; st.eos_id = e->cfg.eos_id; st.pad_id = e->cfg.pad_id;
        st.rowmap = a->rowmap;
        st.scores = d_scores;
        st.alt_ids = d_alt_ids; st.alt_logp = d_alt_logp;
        st.tok_mask = d_tok_mask; st.set_of_row = d_set_of_row;
        st.row_mask = d_row_mask; st.base_mask = d_base_mask; st.base_set_of_row = d_base_set_of_row; st.ngram_of_row = d_ngram_of_row;
        st.prefix = d_prefix; st.prefix_len = d_prefix_len; st.prefix_ld = prefix_ld; st.tgt_val = d_tgt_val;
        DecTokenArgs t{};
        t.aut = o.aut;
        t.slabs = a->slabs; t.nslab = first ? 0 : a->nslab; t.slab_stride = (long long)a->n * e->V;
        t.vbias = a->vbias ? a->vbias : e->w.bv;
        t.cand_val = a->cand_val; t.cand_idx = a->cand_idx; t.ncand = first ? 0 : std::max(a->ncand, 0);
        t.cand_sum = d_cand_sum;
        t.top_val = d_top_val; t.top_idx = d_top_idx;
        t.x_f32 = a->x_f32; t.x_t = a->x_t;
        if (a->cache && a->cache_fp8) { t.cache8 = reinterpret_cast<uint8_t*>(a->cache); t.inv8 = a->inv_sx; }
        else t.cache = a->cache;
        t.cstride = (long long)e->cfg.max_len * e->D;
        dispatch(e, [&](auto tag) {
            using T_ = decltype(tag);
            if (first) launch_dec_token<T_, true>(e, st, t, a->n);
            else launch_dec_token<T_, false>(e, st, t, a->n);
        });
    });
}

int mocr_op_dec_token_ngram(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                            const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                            const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                            const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}, {d_top_val, d_top_idx, d_alt_ids, d_alt_logp}, {d_tok_mask, d_set_of_row},
                                      {d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row}});
}

int mocr_op_dec_token_prefix(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                             const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                             const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                             const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                             const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}, {d_top_val, d_top_idx, d_alt_ids, d_alt_logp}, {d_tok_mask, d_set_of_row},
                                      {d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row}, {d_prefix, d_prefix_len, prefix_ld, d_tgt_val}});
}

int mocr_op_dec_token_automaton(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                                const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                                const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                                const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                                const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val,
                                const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                                const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}, {d_top_val, d_top_idx, d_alt_ids, d_alt_logp}, {d_tok_mask, d_set_of_row},
                                      {d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row}, {d_prefix, d_prefix_len, prefix_ld, d_tgt_val},
                                      {{{d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state}}}});
}

int mocr_op_dec_token_soft(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                           const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                           const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                           const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                           const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val,
                           const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                           const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state,
                           const float* d_edge_weight, const int32_t* d_default_next) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}, {d_top_val, d_top_idx, d_alt_ids, d_alt_logp}, {d_tok_mask, d_set_of_row},
                                      {d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row}, {d_prefix, d_prefix_len, prefix_ld, d_tgt_val},
                                      {{{d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state}, d_edge_weight,
                                        d_default_next}}});
}

int mocr_op_dec_token_penalty(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                              const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                              const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                              const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                              const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val,
                              const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                              const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state,
                              const float* d_edge_weight, const int32_t* d_default_next, uint32_t* d_seen_mask,
                              const float* d_penalty_of_row) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}, {d_top_val, d_top_idx, d_alt_ids, d_alt_logp}, {d_tok_mask, d_set_of_row},
                                      {d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row}, {d_prefix, d_prefix_len, prefix_ld, d_tgt_val},
                                      {{{d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state}, d_edge_weight,
                                        d_default_next}, {d_seen_mask, d_penalty_of_row}}});
}

int mocr_op_penalty_init(mocr_engine* e, uint32_t* d_seen_mask, int32_t rows) {
    return op_hook(e, [&] {
        if (!e->committed || !d_seen_mask || rows < 1 || e->V % 32) throw ArgError{"mocr_op_penalty_init: bad argument", MOCR_ERR_ARG};
        launch_penalty_init(e, d_seen_mask, rows);
    });
}

static int op_automaton_init(mocr_engine* e, uint32_t* d_row_mask, const uint32_t* d_base_mask, const int32_t* d_base_set_of_row,
                             const int32_t* d_ngram_of_row, int32_t rows, const int32_t* d_edge_begin, const int32_t* d_edge_token,
                             const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state,
                             const int32_t* d_default_next) {
    return op_hook(e, [&] {
        if (!e->committed || !d_row_mask || !d_base_mask || !d_base_set_of_row || !d_ngram_of_row || rows < 1 || e->V != 6144 ||
            !d_edge_begin || !d_edge_token || !d_accepting || !d_aut_base_of_row || !d_aut_state)
            throw ArgError{"mocr_op_automaton_init: bad argument", MOCR_ERR_ARG};
        launch_automaton_init(e, d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, rows, d_edge_begin, d_edge_token, d_accepting,
                              d_aut_base_of_row, d_aut_state, d_default_next);
    });
}

int mocr_op_automaton_init_soft(mocr_engine* e, uint32_t* d_row_mask, const uint32_t* d_base_mask, const int32_t* d_base_set_of_row,
                                const int32_t* d_ngram_of_row, int32_t rows, const int32_t* d_edge_begin, const int32_t* d_edge_token,
                                const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state,
                                const int32_t* d_default_next) {
    return op_automaton_init(e, d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, rows, d_edge_begin, d_edge_token, d_accepting,
                             d_aut_base_of_row, d_aut_state, d_default_next);
}

int mocr_op_automaton_init(mocr_engine* e, uint32_t* d_row_mask, const uint32_t* d_base_mask, const int32_t* d_base_set_of_row,
                           const int32_t* d_ngram_of_row, int32_t rows, const int32_t* d_edge_begin, const int32_t* d_edge_token,
                           const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state) {
    return op_automaton_init(e, d_row_mask, d_base_mask, d_base_set_of_row, d_ngram_of_row, rows, d_edge_begin, d_edge_token, d_accepting,
                             d_aut_base_of_row, d_aut_state, nullptr);
}

int mocr_op_dec_token_masked(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                             const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                             const uint32_t* d_tok_mask, const int32_t* d_set_of_row) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}, {d_top_val, d_top_idx, d_alt_ids, d_alt_logp}, {d_tok_mask, d_set_of_row}});
}

int mocr_op_dec_token_topk(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                           const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}, {d_top_val, d_top_idx, d_alt_ids, d_alt_logp}});
}

int mocr_op_dec_token_scored(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores) {
    return op_dec_token(e, a, TokenOp{{d_cand_sum, d_scores}});
}

int mocr_op_dec_token(mocr_engine* e, const mocr_token_args* a) { return op_dec_token(e, a); }

// The fused LM head on the caller's buffers: the four mocr_op_gemm_argmax* / _topk symbols are this with some of `lm` null.
static int op_lm_head(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val, int32_t M, int32_t N,
                      int32_t K, int32_t tile, const LmHead& lm) {
    int32_t* const d_cand_idx = lm.cand_idx;
    float* const d_cand_sum = lm.cand_sum, * const d_top_val = lm.top_val;
    int32_t* const d_top_idx = lm.top_idx;
    const uint32_t* const d_tok_mask = lm.mask.table;
    const int32_t* const d_set_of_row = lm.mask.set_of_row;
    return op_hook(e, [&] {
        if (!e->committed || !dA || !dW || !d_bias || !d_cand_val || !d_cand_idx || M < 1 || K < 1 || (tile != 64 && tile != 128))
            throw ArgError{"mocr_op_gemm_argmax: bad argument", MOCR_ERR_ARG};
        if ((d_top_val == nullptr) != (d_top_idx == nullptr) || (d_top_val && !d_cand_sum))
            throw ArgError{"mocr_op_gemm_topk: d_top_val / d_top_idx come together and with d_cand_sum", MOCR_ERR_ARG};
        if ((d_tok_mask == nullptr) != (d_set_of_row == nullptr) || (d_tok_mask && N % 128))
            throw ArgError{"mocr_op_gemm_argmax_masked: d_tok_mask and d_set_of_row come together, N a multiple of 128", MOCR_ERR_ARG};
        const TokTarget& tt = lm.target;
        if ((tt.prefix || tt.prefix_len || tt.step || tt.tgt_val) &&
            (!tt.prefix || !tt.prefix_len || !tt.step || !tt.tgt_val || tt.prefix_ld < 1 || !d_tok_mask || !d_cand_sum))
            throw ArgError{"mocr_op_gemm_argmax_target: the five target arrays come together, with d_tok_mask and d_cand_sum", MOCR_ERR_ARG};
        const TokSoft& ts = lm.soft;
        if ((ts.state || ts.edge_begin || ts.edge_token || ts.edge_weight) &&
            (!ts.state || !ts.edge_begin || !ts.edge_token || !ts.edge_weight || !d_tok_mask))
            throw ArgError{"mocr_op_gemm_argmax_soft: the states and the three tables come together, with d_tok_mask", MOCR_ERR_ARG};
        const TokPen& tp = lm.pen;
        if ((tp.seen_mask || tp.penalty_of_row) && (!tp.seen_mask || !tp.penalty_of_row || !d_tok_mask))
            throw ArgError{"mocr_op_gemm_argmax_penalty: d_seen_mask and d_penalty_of_row come together, with d_tok_mask", MOCR_ERR_ARG};
        // (the name and the epilogue by the richest output given, as the steps choose theirs by the batch's mode)
        DecMode m;
        m.level = d_top_val ? 2 : d_cand_sum ? 1 : 0; m.mask = d_tok_mask != nullptr;
        const char* const name = m.mask ? "op_gemm_argmax_masked" : m.level == 2 ? "op_gemm_topk" : m.level == 1 ? "op_gemm_argmax_lse" : "op_gemm_argmax";
        GemmCall c = gemm_call(name, dA, K, dW, d_bias, d_cand_val, N, M, N, K, m.epilogue(), tile);
        c.lm = &lm;
        dispatch(e, [&](auto tag) { gemm<decltype(tag)>(e, c); });
    });
}

int mocr_op_gemm_argmax_masked(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                               int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                               int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                               const int32_t* d_rowmap) {
    return op_lm_head(e, dA, dW, d_bias, d_cand_val, M, N, K, tile,
                      LmHead{d_cand_idx, d_cand_sum, d_top_val, d_top_idx, TokMask{d_tok_mask, d_set_of_row, d_rowmap}});
}

int mocr_op_gemm_argmax_target(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                               int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                               int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                               const int32_t* d_rowmap, const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld,
                               const int32_t* d_step, float* d_tgt_val) {
    return op_lm_head(e, dA, dW, d_bias, d_cand_val, M, N, K, tile,
                      LmHead{d_cand_idx, d_cand_sum, d_top_val, d_top_idx, TokMask{d_tok_mask, d_set_of_row, d_rowmap},
                             TokTarget{d_prefix, d_prefix_len, prefix_ld, d_step, d_tgt_val}});
}

// a caller's mocr_soft_tables (null: none) as the LM head takes them; false: not the struct this library knows
static bool soft_tables(const mocr_soft_tables* soft, TokSoft& ts) {
    if (soft && soft->struct_size != (int32_t)sizeof(mocr_soft_tables)) return false;
    if (soft) ts = TokSoft{soft->d_aut_state, soft->d_edge_begin, soft->d_edge_token, soft->d_edge_weight};
    return true;
}

int mocr_op_gemm_argmax_soft(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                             int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                             int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                             const int32_t* d_rowmap, const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld,
                             const int32_t* d_step, float* d_tgt_val, const mocr_soft_tables* soft) {
    TokSoft ts{};
    if (!soft_tables(soft, ts)) return MOCR_ERR_ARG;
    return op_lm_head(e, dA, dW, d_bias, d_cand_val, M, N, K, tile,
                      LmHead{d_cand_idx, d_cand_sum, d_top_val, d_top_idx, TokMask{d_tok_mask, d_set_of_row, d_rowmap},
                             TokTarget{d_prefix, d_prefix_len, prefix_ld, d_step, d_tgt_val}, ts});
}

int mocr_op_gemm_argmax_penalty(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                                int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                                int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                                const int32_t* d_rowmap, const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld,
                                const int32_t* d_step, float* d_tgt_val, const mocr_soft_tables* soft, const uint32_t* d_seen_mask,
                                const float* d_penalty_of_row) {
    TokSoft ts{};
    if (!soft_tables(soft, ts)) return MOCR_ERR_ARG;
    return op_lm_head(e, dA, dW, d_bias, d_cand_val, M, N, K, tile,
                      LmHead{d_cand_idx, d_cand_sum, d_top_val, d_top_idx, TokMask{d_tok_mask, d_set_of_row, d_rowmap},
                             TokTarget{d_prefix, d_prefix_len, prefix_ld, d_step, d_tgt_val}, ts, TokPen{d_seen_mask, d_penalty_of_row}});
}

int mocr_op_gemm_topk(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                      int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N, int32_t K,
                      int32_t tile) {
    return op_lm_head(e, dA, dW, d_bias, d_cand_val, M, N, K, tile, LmHead{d_cand_idx, d_cand_sum, d_top_val, d_top_idx, {}});
}

int mocr_op_gemm_argmax_lse(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                            int32_t* d_cand_idx, float* d_cand_sum, int32_t M, int32_t N, int32_t K, int32_t tile) {
    return op_lm_head(e, dA, dW, d_bias, d_cand_val, M, N, K, tile, LmHead{d_cand_idx, d_cand_sum, nullptr, nullptr, {}});
}

int mocr_op_gemm_argmax(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                        int32_t* d_cand_idx, int32_t M, int32_t N, int32_t K, int32_t tile) {
    return op_lm_head(e, dA, dW, d_bias, d_cand_val, M, N, K, tile, LmHead{d_cand_idx, nullptr, nullptr, nullptr, {}});
}

int mocr_op_smallm_gemm(mocr_engine* e, const mocr_smallm_args* a) {
    return op_hook(e, [&] {
        if (!a || a->struct_size != (int32_t)sizeof(mocr_smallm_args)) throw ArgError{"mocr_op_smallm_gemm: bad struct_size", MOCR_ERR_ARG};
        if (!e->committed || e->cfg.dtype != MOCR_BF16 || !a->w || !a->out || a->rows < 1 || a->N < 1 || a->ldo < a->N ||
            (a->pro == SM_PRO_PLAIN && !a->a_bf16) || (a->pro == SM_PRO_LN && (!a->a_f32 || !a->ln_g || !a->ln_b)) ||
            (a->epi != SM_EPI_RAW && !a->bias) || (a->epi == SM_EPI_SUM && !a->resid) ||
            (a->resid_stats && (!a->resid_g || !a->resid_b)))
            throw ArgError{"mocr_op_smallm_gemm: bad argument", MOCR_ERR_ARG};
        SmallMParams p{};
        p.a_bf16 = reinterpret_cast<const bf16_t*>(a->a_bf16); p.a_f32 = a->a_f32; p.ln_g = a->ln_g; p.ln_b = a->ln_b;
        p.stats_out = a->stats_out; p.w = reinterpret_cast<const bf16_t*>(a->w); p.bias = a->bias; p.resid = a->resid;
        p.resid_stats = a->resid_stats; p.resid_g = a->resid_g; p.resid_b = a->resid_b; p.out = a->out; p.ldo = a->ldo;
        p.rows = a->rows; p.K = a->K; p.N = a->N;
        if (!smallm_pair_exists(a->pro, a->epi))
            throw ArgError{"mocr_op_smallm_gemm: (pro, epi) is not a pair the small-batch decode step launches", MOCR_ERR_UNSUPPORTED};
        smallm_gemm(e, "op_smallm", a->pro, a->epi, p);
    });
}

int mocr_op_latent_block(mocr_engine* e, const mocr_latent_args* a) {
    return op_hook(e, [&] {
        if (!a || a->struct_size != (int32_t)sizeof(mocr_latent_args)) throw ArgError{"mocr_op_latent_block: bad struct_size", MOCR_ERR_ARG};
        if (!e->committed || e->cfg.dtype != MOCR_BF16 || e->D != 768 || e->H != 12 || a->n < 1 || a->regime_rows < 0 ||
            !a->x_in || !a->wq || !a->bq || !a->wkT || !a->wv || !a->bv || !a->keys || !a->q || !a->qt || !a->et || !a->ctx ||
            a->key_stride < 1 || (a->self && !a->step) || (!a->self && a->fixed_len < 1) || (e->fp8attn && !(a->sx > 0.f)))
            throw ArgError{"mocr_op_latent_block: bad argument", MOCR_ERR_ARG};
        LatentBlockArgs b{};
        b.self = a->self != 0; b.n = a->n; b.approx_len = b.self ? e->cfg.max_len : a->fixed_len;
        b.xin = a->x_in; b.wq = a->wq; b.bq = a->bq; b.wkT = a->wkT; b.wv = a->wv; b.bv = a->bv;
        b.keys = a->keys; b.key_stride = a->key_stride; b.fixed_len = b.self ? 0 : a->fixed_len;
        b.step = b.self ? a->step : nullptr; b.rowmap = a->rowmap; b.sx = e->fp8attn ? a->sx : 0.f;
        b.q = a->q; b.qt = a->qt; b.et = a->et; b.ctx = a->ctx;
        // the choices are made by the batch's regime, as in the decode step (which sets it around a batch's steps)
        RegimeScope rs(e, a->regime_rows);
        launch_latent_block(e, b);
    });
}

int mocr_profile_enable(mocr_engine* e, int32_t on) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->prof_collect();
        e->prof_on = on != 0;
    });
}

int mocr_profile_reset(mocr_engine* e) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->prof_collect();
        for (auto& s : e->stats) { s.launches = 0; s.total_ms = 0; s.flops = 0; s.bytes = 0; }
    });
}

int mocr_profile_get(mocr_engine* e, mocr_kernel_stat* out, int32_t cap, int32_t* n_out) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!out || !n_out || cap < 0) throw ArgError{"bad argument", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        e->prof_collect();
        int k = 0;
        for (auto& s : e->stats)
            if (s.launches > 0 && k < cap) out[k++] = s;
        *n_out = k;
    });
}

int mocr_op_beam_select(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score, int32_t* d_parent,
                        int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open) {
    return mocr_op_beam_select_positions(e, a, beam, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, nullptr);
}

int mocr_op_beam_select_tokens(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score,
                               int32_t* d_parent, int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open,
                               float* d_beam_logp, float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row) {
    return mocr_op_beam_select_positions(e, a, beam, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open, d_beam_logp,
                                         d_hyp_logp, d_tok_mask, d_set_of_row, nullptr, nullptr);
}

int mocr_op_beam_select_positions(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score,
                                  int32_t* d_parent, int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open,
                                  float* d_beam_logp, float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                                  uint8_t* d_beam_trail, uint8_t* d_hyp_trail) {
    return mocr_op_beam_select_automaton(e, a, beam, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open, d_beam_logp,
                                         d_hyp_logp, d_tok_mask, d_set_of_row, d_beam_trail, d_hyp_trail, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr);
}

int mocr_op_beam_select_automaton(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score,
                                  int32_t* d_parent, int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open,
                                  float* d_beam_logp, float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                                  uint8_t* d_beam_trail, uint8_t* d_hyp_trail, const int32_t* d_edge_begin, const int32_t* d_edge_token,
                                  const int32_t* d_edge_next, const uint8_t* d_accepting, const int32_t* d_aut_base_of_row,
                                  int32_t* d_aut_state, int32_t* d_hyp_state) {
    return mocr_op_beam_select_soft(e, a, beam, d_beam_score, d_parent, d_hyp_ids, d_hyp_len, d_hyp_score, d_heuristic_open, d_beam_logp,
                                    d_hyp_logp, d_tok_mask, d_set_of_row, d_beam_trail, d_hyp_trail, d_edge_begin, d_edge_token, d_edge_next,
                                    d_accepting, d_aut_base_of_row, d_aut_state, d_hyp_state, nullptr, nullptr);
}

int mocr_op_beam_select_soft(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score, int32_t* d_parent,
                             int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open, float* d_beam_logp,
                             float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint8_t* d_beam_trail,
                             uint8_t* d_hyp_trail, const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                             const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state, int32_t* d_hyp_state,
                             const float* d_edge_weight, const int32_t* d_default_next) {
    return op_hook(e, [&] {
        if (!a || a->struct_size != (int32_t)sizeof(mocr_token_args)) throw ArgError{"mocr_op_beam_select: bad struct_size", MOCR_ERR_ARG};
        if (!e->committed || !beam || beam->num_beams < 2 || beam->num_beams > MOCR_MAX_BEAMS || beam->early_stopping < 0 ||
            beam->early_stopping > 2 || beam->no_repeat_ngram_size < 0 || a->first || a->forced || a->ncand > 0 || a->n < 1 || !a->slabs ||
            a->nslab < 1 || !a->ids || !a->step || !a->finished || !a->len || !a->n_unfinished || !a->rowmap || !a->x_f32 || !a->x_t ||
            a->ids_ld < 2 || a->ids_ld > BEAM_HIST || a->max_len < 2 || a->max_len > a->ids_ld || a->max_len > e->cfg.max_len ||
            !d_beam_score || !d_parent || !d_hyp_ids || !d_hyp_len || !d_hyp_score || !d_heuristic_open)
            throw ArgError{"mocr_op_beam_select: bad argument", MOCR_ERR_ARG};
        const void* const aut_ptrs[7] = {d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state, d_hyp_state};
        for (const void* p : aut_ptrs)
            if ((p == nullptr) != (d_aut_state == nullptr))
                throw ArgError{"mocr_op_beam_select_automaton: the seven automaton pointers must be all null or all set", MOCR_ERR_ARG};
        if ((d_edge_weight == nullptr) != (d_default_next == nullptr) || (d_edge_weight && !d_aut_state))
            throw ArgError{"mocr_op_beam_select_soft: d_edge_weight and d_default_next come as a pair, with the seven automaton pointers", MOCR_ERR_ARG};
        DecState st{};
        st.n_real = a->n_real;
        st.ids = a->ids; st.step = a->step; st.finished = a->finished; st.len = a->len; st.n_unfinished = a->n_unfinished;
        st.ids_ld = a->ids_ld; st.max_len = a->max_len;
        st.start_id = e->cfg.start_id; st.eos_id = e->cfg.eos_id; st.pad_id = e->cfg.pad_id;
        st.rowmap = a->rowmap;
        BeamState bs{};
        bs.beam_score = d_beam_score; bs.parent = d_parent; bs.hyp_ids = d_hyp_ids; bs.hyp_len = d_hyp_len; bs.hyp_score = d_hyp_score;
        bs.heuristic_open = d_heuristic_open;
        bs.beam_logp = d_beam_logp; bs.hyp_logp = d_hyp_logp; bs.tok_mask = d_tok_mask; bs.set_of_row = d_set_of_row;
        bs.beam_trail = d_beam_trail; bs.hyp_trail = d_hyp_trail;      // (launch_beam_select refuses one without the other)
        bs.length_penalty = beam->length_penalty; bs.early_stopping = beam->early_stopping; bs.ngram = beam->no_repeat_ngram_size;
        DecTokenArgs t{};
        t.slabs = a->slabs; t.nslab = a->nslab; t.slab_stride = (long long)a->n * e->V;
        t.vbias = a->vbias ? a->vbias : e->w.bv;
        t.x_f32 = a->x_f32; t.x_t = a->x_t;
        if (a->cache && a->cache_fp8) { t.cache8 = reinterpret_cast<uint8_t*>(a->cache); t.inv8 = a->inv_sx; }
        else t.cache = a->cache;
        t.cstride = (long long)e->cfg.max_len * e->D;
        BeamSoftAutomata aut{};
        static_cast<BeamAutomata&>(aut) = BeamAutomata{d_edge_begin, d_edge_token, d_edge_next, d_accepting, d_aut_base_of_row, d_aut_state, d_hyp_state};
        aut.edge_weight = d_edge_weight; aut.default_next = d_default_next;
        dispatch(e, [&](auto tag) { launch_beam_select<decltype(tag)>(e, st, bs, t, a->n, beam->num_beams, aut); });
    });
}

int mocr_op_beam_permute(mocr_engine* e, void* d_cache, int32_t layers, int64_t layer_stride, int64_t row_stride, int32_t segs,
                         int64_t seg_stride, int32_t pos_bytes, int32_t K, const int32_t* d_parent, const int32_t* d_rowmap,
                         const int32_t* d_finished, const int32_t* d_step, int32_t n_slots, int32_t max_pos) {
    return op_hook(e, [&] {
        if (!d_cache || !d_parent || !d_rowmap || !d_finished || !d_step || n_slots < 1 || K < 2 || K > MOCR_MAX_BEAMS || layer_stride < 0 ||
            row_stride < 16 || seg_stride < 0 || layer_stride % 16 || row_stride % 16 || seg_stride % 16 ||
            (reinterpret_cast<uintptr_t>(d_cache) & 15))
            throw ArgError{"mocr_op_beam_permute: bad argument", MOCR_ERR_ARG};
        BeamPermuteView v{reinterpret_cast<char*>(d_cache), layer_stride, row_stride, seg_stride, segs, pos_bytes};
        launch_beam_permute(e, v, layers, K, d_parent, d_rowmap, d_finished, d_step, n_slots, max_pos);
    });
}

int64_t mocr_beam_state_bytes(mocr_engine* e) {
    return beam_group_bytes(e, [](const LaneCtx& c) { return c.hyp_ids != nullptr; }, beam_state_arrays);
}

int64_t mocr_beam_token_state_bytes(mocr_engine* e) {
    return beam_group_bytes(e, [](const LaneCtx& c) { return c.hyp_logp != nullptr; }, beam_token_arrays);
}

int64_t mocr_beam_position_state_bytes(mocr_engine* e) {
    return beam_group_bytes(e, [](const LaneCtx& c) { return c.hyp_trail != nullptr; }, beam_position_arrays);
}

int mocr_lane_rowmap(mocr_engine* e, int32_t lane, int32_t* out_rowmap, int32_t n) {
    return guarded(e, [&] {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!out_rowmap || lane < 0 || lane >= (int)e->lanes.size() || n < 1 || n > e->Bp) throw ArgError{"mocr_lane_rowmap: bad argument", MOCR_ERR_ARG};
        HIPCHECK(hipSetDevice(e->cfg.device));
        drive(e);
        HIPCHECK(hipMemcpy(out_rowmap, e->lanes[lane].ctx.rowmap, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
