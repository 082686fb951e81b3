/*
 * mocr.h - C ABI of the MI355X-native Manga-OCR recogniser engine (libmocr_hip.so).
 *
 * This is the drop-in boundary for ONE call of the reference application:
 *
 *     raw_text = self.manga_ocr_reader(pil_img)          reference src/ui/main_window.py:9801
 *
 * i.e. `manga_ocr.MangaOcr.__call__(PIL.Image) -> str`, constructed once at
 * src/ui/main_window.py:3394 (`MangaOcr()`), imported at src/core/config.py:431-436 and
 * called concurrently, without a lock, by up to MAX_WORKERS QueueProcessorWorker threads
 * (src/core/workers.py:209-247, 318-327, 383-402) and by the text-detect path
 * (src/ui/main_window.py:9462-9476, 9530-9549).  The reference has no native interface of
 * its own (it is pure Python); the entry points below are what a binding for that call
 * needs, and the Python class manga_ocr.MangaOcr in this repo is that binding (ctypes).
 * INTEGRATION.md shows the stub.
 *
 * Conventions: plain C, no exceptions, no Python or torch types.  Every function returns
 * MOCR_OK (0) or a negative error code; mocr_last_error() returns a message for the last
 * failure on that engine.  The caller owns every buffer it passes.  Token-id blocks are
 * int32, row-major [n, max_len]; a row holds start_id, the generated ids, eos_id, then
 * pad_id up to max_len - exactly the rows `generate(max_length=max_len)` returns
 * (TF/generation/utils.py:2929-2937), padded to the fixed width.
 */
#ifndef MOCR_H
#define MOCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOCR_ABI_VERSION 2      /* 2: mocr_image.rotate (occupies what was padding: the struct keeps its size) */

enum {
    MOCR_OK = 0,
    MOCR_ERR_ARG = -1,          /* bad argument (null, size, unsupported shape) */
    MOCR_ERR_STATE = -2,        /* call order (weights not committed, ...) */
    MOCR_ERR_HIP = -3,          /* a HIP runtime call failed */
    MOCR_ERR_UNSUPPORTED = -4,  /* valid request this build does not implement */
    MOCR_ERR_NOMEM = -5
};

enum { MOCR_F32 = 0, MOCR_BF16 = 1 };

/* mocr_config.flags */
enum {
    MOCR_FLAG_SIMPLE_ATTENTION = 1 << 0, /* encoder attention on the VALU kernel even in bf16 mode */
    MOCR_FLAG_NO_GRAPH = 1 << 1,         /* launch decode steps eagerly instead of replaying a HIP graph */
    MOCR_FLAG_NO_EARLY_EXIT = 1 << 2,    /* always run max_len-1 decode steps */
    MOCR_FLAG_CLASSIC_ATTENTION = 1 << 3, /* bf16: projected K/V caches instead of the latent (absorbed) decode attention */
    MOCR_FLAG_NO_FUSED_ARGMAX = 1 << 4,   /* always write the logits and take the argmax in the token kernel */
    MOCR_FLAG_NO_FUSED_QQT = 1 << 5,      /* latent attention: query and absorbed query as two GEMM launches even for fat batches */
    MOCR_FLAG_FP8_ATTENTION = 1 << 7,     /* bf16 engines, opt-in (BASELINE configs[4]): the latent decode attention reads its
                                           * key/value rows as OCP e4m3 (768 B per key instead of 1,536 B, static per-source
                                           * scales) and runs both products on fp8 MFMA, softmax in fp32.  NOT the parity
                                           * configuration: its accuracy is reported by tests/test_gpu_fp8_attention.py */
    MOCR_FLAG_LATENT_ALWAYS = 1 << 6,     /* bf16: latent attention for every batch size (default: batches of <= 256 rows take the
                                           * classic projected-K/V kernels, whose grid - one block per (row, head) - has half the
                                           * step latency there: 50 instead of 80 ms for 64 crops) */
    MOCR_FLAG_NO_SMALL_BATCH_PATH = 1 << 8, /* bf16: batches of <= 32 rows through the generic split-K projections + add/LayerNorm
                                           * launches (28 per decode step) instead of the one-launch-per-projection path (19) */
    MOCR_FLAG_LATENT_TILE32 = 1 << 10,    /* bf16 latent attention on r03's kernel shape (32-key tiles, one persistent block per CU, three
                                           * barriers per tile) instead of the default, latent_attnT_kernel<., 2>: 16-key tiles on three
                                           * blocks per CU with the score tile transposed (two barriers per tile): the A/B partner */
    MOCR_FLAG_NO_COMPACTION = 1 << 11,    /* keep every row of a batch in the decode steps until the whole batch has finished (r01-r03
                                           * behaviour) instead of compacting the unfinished rows between chunks of steps */
    MOCR_FLAG_FORCE_LN_FOLD = 1 << 13,    /* bf16: fold the encoder's LayerNorms even where this checkpoint's residual stream failed the
                                           * commit-time check (mocr_ln_fold_state): A/B and tests only */
    MOCR_FLAG_NO_LN_FOLD = 1 << 9         /* bf16: the encoder's LayerNorms as launches of their own even where the layer GEMMs run on
                                           * the persistent kernel (default there: folded into the GEMMs on both sides of them) */
};

typedef struct mocr_engine mocr_engine;

/* Replaces the (argument-less) constructor call at src/ui/main_window.py:3394.  The model
 * hyper-parameters are those BASELINE.json fixes (ViT-B/16-224 + 2-layer BERT decoder). */
typedef struct mocr_config {
    int32_t struct_size; /* sizeof(mocr_config), for forward compatibility */
    int32_t device;      /* HIP device ordinal of this process's GPU */
    int32_t dtype;       /* MOCR_F32 (parity mode) or MOCR_BF16 (bf16 storage, fp32 accumulate) */
    int32_t max_batch;   /* crops per internal batch (rows of one decode step) */
    int32_t max_len;     /* generate(max_length): 300 */
    int32_t image_size;  /* 224 */
    int32_t patch_size;  /* 16 */
    int32_t hidden;      /* 768 */
    int32_t enc_layers;  /* 12 */
    int32_t dec_layers;  /* 2 */
    int32_t heads;       /* 12 */
    int32_t ffn;         /* 3072 */
    int32_t vocab;       /* 6144 */
    int32_t max_pos;     /* 512 */
    int32_t start_id;    /* 2 */
    int32_t eos_id;      /* 3 */
    int32_t pad_id;      /* 0 */
    float ln_eps;        /* 1e-12 */
    int32_t flags;
    int32_t lanes;       /* batches kept in flight on separate HIP streams (0 = 1); each has its own workspace */
} mocr_config;

int mocr_abi_version(void);

/* Construct an engine on cfg->device.  Allocates all device memory for max_batch. */
int mocr_create(const mocr_config* cfg, mocr_engine** out);
void mocr_destroy(mocr_engine* e);
const char* mocr_last_error(const mocr_engine* e);

/* Weights: one call per tensor of the model (canonical transformers-5.x state_dict names,
 * e.g. "encoder.layers.0.attention.q_proj.weight"), host float32, row-major; then commit.
 * Replaces the `from_pretrained(...)` inside the reference's recogniser constructor. */
int mocr_set_tensor(mocr_engine* e, const char* name, const float* data, const int64_t* shape, int32_t ndim);
int mocr_commit_weights(mocr_engine* e);

/* THE HOT PATH (host buffers).  images: n crops, uint8, each h x w with `channels` (1 = the
 * luminance plane the recogniser's convert('L') would produce, 3 = RGB as handed over at
 * src/ui/main_window.py:9800; converted on the device with Pillow's fixed-point formula),
 * row_stride bytes between rows, image_stride bytes between crops.  h and w must equal
 * image_size (crops of other sizes: mocr_recognize_images below).
 * out_ids [n, max_len] int32, out_len [n] int32.  Blocking; thread-safe (calls from
 * several threads are serialised per engine).  n may exceed max_batch. */
int mocr_recognize(mocr_engine* e, const uint8_t* images, int32_t n, int32_t h, int32_t w,
                   int64_t row_stride, int64_t image_stride, int32_t channels,
                   int32_t* out_ids, int32_t* out_len);

/* THE HOT PATH from crops of ANY size (BASELINE configs[4]'s variable-resolution crops).
 * The device does what the reference's recogniser and image processor do in front of the encoder:
 * img.convert('L') [.convert('RGB')] and resize((224,224), BILINEAR) (MangaOcr.__call__, SURVEY row a10;
 * TF/models/vit/image_processing_pil_vit.py:20-27, TF/image_processing_backends.py:521-570 -> Pillow's
 * ImagingResample) - in Pillow's own fixed-point arithmetic, i.e. bit-exact with the CPU path.
 * One descriptor per crop: host pointer, size, bytes between rows, channels (1 = L, 3 = RGB as handed over at
 * src/ui/main_window.py:9800).  The callee neither keeps nor modifies the pixels. */
typedef struct mocr_image {
    const uint8_t* data;
    int32_t height, width;
    int64_t row_stride;
    int32_t channels;   /* 1 = L, 3 = RGB, MOCR_CHANNELS_BGR = 3 bytes per pixel in OpenCV's B,G,R order */
    int32_t rotate;     /* MOCR_ROTATE_NONE, or the reference's orientation-only rotation applied ON THE DEVICE before the
                         * resize: MOCR_ROTATE_90_CW = cv2.ROTATE_90_CLOCKWISE ("Vertical" setting, landscape crop),
                         * MOCR_ROTATE_90_CCW = cv2.ROTATE_90_COUNTERCLOCKWISE ("Horizontal" setting, portrait crop);
                         * src/core/workers.py:320-326, src/ui/main_window.py:9787-9795.  height / width / row_stride
                         * describe the crop as it lies in memory (before the rotation).  Ignored for pages of
                         * mocr_recognize_regions. */
} mocr_image;
enum { MOCR_ROTATE_NONE = 0, MOCR_ROTATE_90_CW = 1, MOCR_ROTATE_90_CCW = 2 };
/* BGR pixels as the reference's crop tools and pages hold them (`cropped_cv_img`, `cv_image`: src/ui/main_window.py:6431,
 * src/core/workers.py:461): the BGR -> RGB swap of src/ui/main_window.py:9800 is folded into the luminance conversion. */
#define MOCR_CHANNELS_BGR (-3)
/* out_ids [n, max_len] int32, out_len [n] int32 (host).  Blocking, thread-safe; n may exceed max_batch. */
int mocr_recognize_images(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len);
/* THE HOT PATH for the Text-detect callers: whole pages plus the bounding
 * rectangles of the regions a detector found on them, replacing the serial loop of `_collect_manga_detections` ->
 * `_recognize_polygon` -> `perform_ocr` (src/ui/main_window.py:9462-9476, 9530-9549, 9774-9803) and, over several
 * pages, of `AutoDetectorWorker.run` (src/core/workers.py:448-482).  Every page is uploaded ONCE; each region's crop -
 * its rectangle grown by int(max(w, h) * 0.08) on every side and clipped to the page, the rule of
 * src/ui/main_window.py:9533-9537 - is cut on the device by the resize kernel's descriptor (offset + page stride), and
 * all regions of all pages decode as one job queue.  A region that leaves no more than a 1-pixel sliver gets
 * out_len = 0 and a row of pad_id (the reference returns '' for it without calling the recogniser, :9538-9539).
 * region.{x, y, width, height} = QPolygon.boundingRect() of the detected polygon, in page pixels. */
typedef struct mocr_region {
    int32_t page;                /* index into pages[] */
    int32_t x, y, width, height;
} mocr_region;
int mocr_recognize_regions(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                           int32_t n_regions, int32_t* out_ids, int32_t* out_len);

/* ---- token scores ---------------------------------------------------------------------------
 * The scored twin of every recognise entry point: one more output, out_logp float32 [n, max_len] with the row layout of
 * out_ids - the log-probability of every emitted token, computed on the device inside the LM-head launch of the step that
 * chose it (the logits still never reach memory):
 *   out_logp[r][0] = 0                      the start token is given, not predicted
 *   out_logp[r][t], 1 <= t < out_len[r]     = logits[ids[r][t]] - logsumexp(logits), logits = the step's fp32 LM-head outputs
 *                                           (acc + bias); softmax in fp32 in both engine dtypes, natural log.  Greedy picks the
 *                                           maximum, so this is -log(sum_j exp(logit_j - max)) <= 0.  The EOS token is scored,
 *                                           and so is the last token of a row that ends by reaching max_len.
 *   out_logp[r][t], t >= out_len[r]         = 0 (the pad tail; a whole row of 0 for a region reduced to a sliver, out_len 0)
 * exp(mean of a row's scores over 1 .. out_len - 1) is the geometric-mean token probability (`Recognition.confidence` of
 * the Python binding).  The ids and lengths are bit-identical to the unscored call's; out_logp = NULL IS the unscored call.
 * Scored and unscored requests may share a batch. */
int mocr_recognize_images_scored(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                 float* out_logp);
int mocr_recognize_regions_scored(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                  int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp);

/* ---- token alternatives -----------------------------------------------------------------------
 * What else a position could have been: the four most probable tokens of every step, from the same LM-head launch that
 * chose the token (the logits still never reach memory: the GEMM epilogue keeps four candidates per tile instead of one).
 * Two more outputs with the row layout of out_ids and one more axis:
 *   out_alt_ids  int32   [n, max_len, MOCR_ALTERNATIVES]
 *   out_alt_logp float32 [n, max_len, MOCR_ALTERNATIVES]
 * For 1 <= t < out_len[r], entry k holds the token with the k-th largest logit of the step that emitted ids[r][t] and its
 * log-probability logit - logsumexp(logits) (fp32 softmax in both engine dtypes, as for the scores).  Entries are ordered by
 * logit descending, equal logits the lower id first - the tie rule of the greedy pick - so
 *   out_alt_ids[r][t][0] == out_ids[r][t], out_alt_logp[r][t][0] is bit-identical to out_logp[r][t],
 *   the four ids of a position are distinct and its four log-probabilities do not increase.
 * For t == 0 and t >= out_len[r] the ids are -1 and the log-probabilities 0 (a whole row of these for a region reduced to a
 * sliver, out_len 0).  Rows without a finite logit are unspecified, as for the scores.
 * Asking for alternatives moves no id and no length.  The two pointers are both null (= the scored call) or both set;
 * out_logp stays nullable.  Unscored, scored and alternatives requests may share a batch; it runs in the richest mode asked.
 * The buffers this needs on the device are allocated by the first request that asks. */
#define MOCR_ALTERNATIVES 4
int mocr_recognize_images_alts(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                               float* out_logp, int32_t* out_alt_ids, float* out_alt_logp);
int mocr_recognize_regions_alts(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                float* out_alt_logp);

/* ---- token constraints ------------------------------------------------------------------------
 * What the caller knows about a crop: a page-number box holds digits, a sound-effect bubble kana, a pipeline never wants
 * [UNK].  A TOKEN SET is a subset of the vocabulary; a crop decoded under a set behaves as if the logits of every other token
 * were -inf before the argmax and before the softmax of EVERY step (the greedy loop feeds each token back, and the logits
 * never reach memory, so the LM-head epilogue and the token kernel apply the set themselves):
 *   ids           the argmax over the set's tokens, equal logits the lowest allowed id;
 *   scores        the log-softmax over the set's tokens only (renormalised);
 *   alternatives  the four best tokens of the set and their renormalised log-probabilities, in the order above, entry 0 the
 *                 emitted id; a set of fewer than four tokens leaves id -1 / log-probability -inf in the missing entries
 *                 (a finished row's positions stay -1 / 0).
 * EOS belongs to every set (the engine adds it); the start token, the pad ids of finished rows and the max_len stop are not
 * constrained, nor is the teacher-forced hook mocr_decode_logits.  Set MOCR_TOKEN_SET_ALL (0) is the whole vocabulary: a row
 * under it, also inside a batch with constrained rows, gives ids, scores and alternatives bit-identical to an unconstrained
 * batch of the same mode and size.  Sets are per crop and one batch may mix any of them (the scheduler merges requests).
 *
 * mocr_token_set_create: ids[n_ids] in [0, vocab), duplicates allowed; *out_set = the handle (>= 1), the existing one when a
 * set of the same content exists.  Sets are immutable and live until mocr_destroy; at most MOCR_MAX_TOKEN_SETS including
 * set 0.  MOCR_ERR_ARG: n_ids <= 0, an id out of range, the table full.  Thread-safe; needs committed weights.
 * mocr_token_set_count: handles in use, set 0 included (valid handles are 0 .. count - 1).
 * The *_constrained entry points: the *_alts twins plus `sets`, a HOST array of one handle per crop (per region), null = all
 * MOCR_TOKEN_SET_ALL; out_logp / out_alt_ids / out_alt_logp nullable as there.  An unknown handle: MOCR_ERR_ARG. */
#define MOCR_MAX_TOKEN_SETS 256
#define MOCR_TOKEN_SET_ALL 0
int mocr_token_set_create(mocr_engine* e, const int32_t* ids, int32_t n_ids, int32_t* out_set);
int mocr_token_set_count(mocr_engine* e);
int mocr_recognize_images_constrained(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                      float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets);
int mocr_recognize_regions_constrained(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                       int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                       float* out_alt_logp, const int32_t* sets);

/* ---- no-repeat n-grams ------------------------------------------------------------------------
 * The published checkpoint's generation config carries no_repeat_ngram_size = 3; under greedy decoding it is what stops a
 * decoder that has fallen into a loop (repeated-character bubbles) from running to max_len.  The rule is that of
 * transformers' NoRepeatNGramLogitsProcessor applied to greedy search.  Per row n = its size, 0 = off.  The row holds L
 * tokens ids[0 .. L-1], the start token included; the step that chooses ids[L] bans a set of tokens:
 *   L + 1 < n   nothing is banned;
 *   otherwise   { ids[i+n-1] : 0 <= i <= L-n and ids[i .. i+n-2] == ids[L-n+1 .. L-1] };
 *   n = 1       the key is empty: every token already in the row is banned, the start token too.
 * A banned token counts as a logit of -inf before the argmax and before the softmax of that step, exactly as a token outside
 * the row's token set does (token constraints, above); the effective set of a step is the row's set minus the bans:
 *   ids           the argmax over what is left, equal logits the lowest id;
 *   scores        and the four alternatives are renormalised over what is left; entry 0 of the alternatives stays the
 *                 emitted id.
 * EOS cannot be banned (an unfinished row's history never holds it), so every step keeps a finite maximum.  The start token,
 * the pad ids of finished rows, the max_len stop and mocr_decode_logits are untouched.  n is per crop and one batch may mix
 * any values (the scheduler merges requests); a row with n = 0 and set MOCR_TOKEN_SET_ALL, also inside a batch with rows
 * that do have bans, gives ids, scores and alternatives bit-identical to an unconstrained batch of the same mode and size.
 * The bans depend on the row's own history, so the engine keeps one effective mask per row on the device and the token
 * kernel rebuilds it after every token, inside the captured decode steps.
 *
 * The *_norepeat entry points: the *_constrained twins plus `ngram`, a HOST array of one size per crop (per region), null =
 * all 0; with `ngram` null they ARE the constrained calls.  A size outside 0 .. the engine's max_len: MOCR_ERR_ARG. */
int mocr_recognize_images_norepeat(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                   float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets,
                                   const int32_t* ngram);
int mocr_recognize_regions_norepeat(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                    int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                    float* out_alt_logp, const int32_t* sets, const int32_t* ngram);

/* ---- token positions ---------------------------------------------------------------------------
 * Where in the crop each token was read: the cross-attention of the LAST decoder layer over the encoder's 14 x 14 patch
 * grid, reduced to a centre, a spread and a mass per token.  One more output with the row layout of out_ids and one more axis,
 *   out_pos float32 [n, max_len, MOCR_POSITION_FIELDS].
 * For 1 <= t < out_len[r], with a_vec = the last layer's LayerNorm-1 output of the step that consumed ids[r][t-1] and emitted
 * ids[r][t] (in the engine's dtype: the row the cross-attention query projection reads), q = a_vec Wq^T + bq and
 * K = ENC[r] Wk^T + bk over the row's 197 encoder outputs (both of that layer):
 *   p_h = softmax_k(q_h . K_h[k] / 8) per head h of 12, in fp32, the maximum subtracted;  a[k] = (1/12) sum_h p_h[k].
 * Key 0 is CLS; key k >= 1 is the patch in grid row i = (k-1) / 14, column j = (k-1) % 14, at u = (j + 0.5) / 14,
 * v = (i + 0.5) / 14.  The fields:
 *   [MOCR_POS_CX]   sum_{k>=1} a[k] u_k / mass          [MOCR_POS_CY]   the same in v
 *   [MOCR_POS_SX]   sqrt(max(0, sum_{k>=1} a[k] u_k^2 / mass - cx^2))    [MOCR_POS_SY]   the same in v
 *   [MOCR_POS_MASS] sum_{k>=1} a[k] - a small mass says that the step looked at CLS and the position means little;
 *                   below 1e-20: cx = cy = 0.5, sx = sy = 0.
 * (The device computes the spread in the equal, better conditioned centred form sqrt(sum_{k>=1} a[k] (u_k - cx)^2 / mass).)
 * Coordinates are fractions of the 224 x 224 plane the encoder sees: AFTER mocr_image.rotate, and for a region inside its
 * padded, clipped rectangle.  For t = 0, for t >= out_len[r] and for every position of a sliver region (out_len 0) the five
 * fields are 0; the EOS position is computed like any other.
 * Asking for positions moves no id, length, score or alternative, and a batch in which nobody asks launches exactly what it
 * launched before: the decode steps of a batch that does ask only record a_vec (768 values per row and step, a store the
 * LayerNorm launch already had), and ONE batched pass computes every position when the batch has finished - each row's keys
 * are read once, not once per step.  Requests with and without positions may share a batch; rows of requests that did not ask
 * get nothing written.  The buffers are allocated by the first request that asks: per lane max_batch (rounded up to 128) x
 * max_len x (768 elements of the engine's dtype + 20 B), plus at most 64 MiB of scratch whatever max_batch is.
 *
 * The *_positions entry points: the *_norepeat twins plus out_pos (a device pointer for mocr_recognize_device_positions); with
 * out_pos null they ARE the norepeat calls. */
#define MOCR_POSITION_FIELDS 5
enum { MOCR_POS_CX = 0, MOCR_POS_CY = 1, MOCR_POS_SX = 2, MOCR_POS_SY = 3, MOCR_POS_MASS = 4 };
int mocr_recognize_images_positions(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                    float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets,
                                    const int32_t* ngram, float* out_pos);
int mocr_recognize_regions_positions(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                     int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                     float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos);

/* ---- forced prefixes ---------------------------------------------------------------------------
 * Score and continue caller-given tokens.  Per crop there is a prefix p[0 .. P-1] of token ids; the start token is NOT part of
 * it and P = 0 means none.  Row r then holds ids[r][0] = start, ids[r][1 + i] = p[i] for i < P, and greedy tokens after that.
 * The step that fills ids[r][t+1] with t < P is a FORCED step: it runs the decoder exactly as a free step does, only the token
 * that is stored and fed back differs.
 *   Stopping: the rules do not change.  A forced EOS finishes the row (out_len = t + 2, then pad); a row that reaches
 *     generate(max_length) finishes there, forced or not.  EOS may appear only as the last prefix token.
 *   Scores: out_logp[r][t+1] of a forced step = logit[p[t]] - logsumexp over the step's EFFECTIVE set (the row's token set minus
 *     its n-gram bans, as in a free step); -inf when p[t] is outside that set - the token is still emitted and fed back.  On the
 *     device (v - gmax) + (-log S), v the forced column's fp32 acc + bias (-inf when masked), gmax and S what the free step
 *     forms; when the forced token IS the step's own pick the free step's expression is used (a -0 score keeps its sign).  A
 *     prefix that is a whole text plus EOS therefore scores the text: sum_t out_logp[r][t] = log p(text | crop).
 *   Alternatives: at a forced step the step's own four best, as if the step were free - entry 0 is what the model would have
 *     chosen, not necessarily ids[r][t+1].
 *   Sets, n-grams, positions: sets and bans apply to the normaliser and to the alternatives of forced steps; forced tokens enter
 *     the row's history, so later bans see them; positions are computed for forced steps like any other.
 *   Bit identity: a row with P = 0, also inside a batch that has prefixed rows, equals the same row of an un-prefixed batch of
 *     the same mode and size in ids, lengths, scores, alternatives and positions; a row whose prefix equals the first P generated
 *     tokens of its own free decode (same batch size and dtype) reproduces that decode bit for bit; a batch in which nobody
 *     passes a prefix launches exactly what it launched before.
 * A batch with a prefixed row runs the masked, scored decode steps (unconstrained rows under MOCR_TOKEN_SET_ALL); an ids-only
 * caller sharing it gets the same ids.  The buffers (per lane max_batch x (max_len + 2) x 4 B) are allocated by the first
 * request that asks.
 *
 * The *_prefix entry points: the *_positions twins plus `prefix`, a HOST int32 array [n][prefix_ld], `prefix_len`, a HOST
 * int32 array [n], and prefix_ld (per region for the regions call; a sliver region ignores its prefix); with `prefix` and
 * `prefix_len` null they ARE the positions calls.  MOCR_ERR_ARG: exactly one of the two null; prefix_len[i] outside
 * 0 .. L - 1, L the call's generate(max_length) (the override of mocr_recognize_gray_host_prefix); prefix_len[i] > prefix_ld;
 * an id outside [0, vocab); EOS before the last prefix position.  The arrays are copied before the call returns. */
int mocr_recognize_images_prefix(mocr_engine* e, const mocr_image* images, int32_t n, int32_t* out_ids, int32_t* out_len,
                                 float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                 float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld);
int mocr_recognize_regions_prefix(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                  int32_t n_regions, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                  float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                  const int32_t* prefix_len, int32_t prefix_ld);

/* ---- shared encodings ---------------------------------------------------------------------------
 * Several decode rows per crop from one encoder pass.  Scoring eight candidate readings of one bubble, or continuing the
 * alternatives of one reading, are eight rows over the same pixels; the *_shared entry points let the caller say so, and the
 * crop is preprocessed and encoded once per internal batch instead of once per row.
 *   `source` is a HOST int32 array [n_rows]: row r decodes image / region / plane number source[r] of the call.  Any order,
 *     repeats are the point.  It is copied before the call returns.
 *   Every output and every per-crop array of the older sections is per ROW here, [n_rows]...: out_ids, out_len, out_logp, the
 *     alternatives, out_pos, and `sets`, `ngram`, `prefix`, `prefix_len`.
 *   Semantics: sharing changes what the encoder is run on, and nothing else.  A call with source = 0, 1, ..., n - 1 is
 *     bit-identical to the prefix call in every output.  A shared row is NOT promised bit-identical to the same crop sent twice:
 *     the encoder's kernel choice - and in bf16 the LayerNorm fold - go by how many crops it runs on; the decode regime goes by
 *     rows as always.  Rows of different calls may still be merged into one batch, and a request that shares and one that does
 *     not may share a batch.  A call of more than max_batch rows is cut in row order; a crop whose rows fall into two internal
 *     batches is encoded once in each, and results do not depend on where the cut falls.
 *   How: the batch's encoder runs on the distinct crops, then one launch (profile name enc_expand) copies every row's encoding
 *     into place - 197 x hidden elements a row - and the decode kernels run on rows as before.  The per-lane row -> crop map
 *     (max_batch x 4 B) is allocated by the first batch that shares; a batch in which nobody shares launches exactly what it
 *     launched before.
 * The *_shared entry points: the *_prefix twins plus n_rows and `source`; with `source` null they require n_rows == the
 * number of images / regions / planes and ARE the prefix calls.  MOCR_ERR_ARG: n_rows < 1; an index outside [0, number of
 * images); an image, region or plane that no row names; for the device call n_rows > max_batch.  A sliver region gives every
 * one of its rows length 0 (ids all pad_id, the other outputs 0, alternative ids -1; prefixes ignored there). */
int mocr_recognize_images_shared(mocr_engine* e, const mocr_image* images, int32_t n_images, int32_t n_rows, const int32_t* source,
                                 int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                 const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                 const int32_t* prefix_len, int32_t prefix_ld);
int mocr_recognize_regions_shared(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                  int32_t n_regions, int32_t n_rows, const int32_t* source, int32_t* out_ids, int32_t* out_len,
                                  float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                  float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld);
/* The device call (see mocr_recognize_device_prefix below): d_gray holds n_planes planes, the outputs n_rows rows. */
int mocr_recognize_device_shared(mocr_engine* e, const void* d_gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                 void* d_out_ids, void* d_out_len, void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp,
                                 const int32_t* sets, const int32_t* ngram, void* d_out_pos, const int32_t* prefix,
                                 const int32_t* prefix_len, int32_t prefix_ld);
/* The host-plane call (see mocr_recognize_gray_host_prefix below). */
int mocr_recognize_gray_host_shared(mocr_engine* e, const uint8_t* gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                    int32_t max_len_override, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                    float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos,
                                    const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld);
/* Crops the recognise calls' batches have put through the encoder since mocr_create (statistic, cumulative like
 * mocr_decode_slot_steps): how a caller sees that sharing happened - 64 for 512 rows over 64 crops in one batch. */
int64_t mocr_encoded_crops(mocr_engine* e);

/* ---- token automata -----------------------------------------------------------------------------
 * Greedy decoding under a constraint that depends on what the row has emitted so far: a lexicon (a trie over token ids) or a
 * pattern.  This is transformers' prefix_allowed_tokens_fn in its history-dependent form, at one decode row per crop whatever
 * the size of the list.
 *   A TOKEN AUTOMATON is a deterministic finite automaton over token ids: states 0 .. n_states - 1, state 0 the start, given
 *     in CSR form - edge_begin [n_states + 1], edge_token / edge_next [n_edges] hold the edges of every state sorted by token,
 *     strictly ascending, and accepting [n_states] one byte per state.  EOS is never an edge token.
 *   A row decoded under an automaton is in a state s: the start state before the first generated token.  At the step that
 *     chooses ids[L]:
 *       the automaton's set A(s) = the edge tokens of s, plus EOS iff s is accepting; A(MOCR_STATE_DEAD) is empty;
 *       the step's effective set = A(s) AND the row's token set, minus the row's n-gram bans - sets and bans exactly as in
 *         the sections above.  The automaton is the only thing that can take EOS away: the engine still adds EOS to every
 *         token set, so EOS survives the intersection exactly when s accepts;
 *       DEAD-END RULE: an empty effective set becomes {EOS} - the row ends there and every step keeps a finite maximum.  The
 *         rule applies to rows under an automaton only;
 *       ids are the arg-max over the effective set (equal logits: the lowest id), scores and the four alternatives are
 *         renormalised over it - word for word the rule of the constrained calls.
 *     After the step, every token stored by a row that was unfinished before the step, and that is not EOS, moves the state:
 *     s' = next(s, tok), or MOCR_STATE_DEAD where s has no such edge.  The last token of a row that ends by
 *     generate(max_length) is included; EOS moves nothing.  Forced prefix tokens walk the automaton like emitted ones: one
 *     outside the effective set scores -inf as before, and one without an edge leaves the row DEAD.  The start token, the pad
 *     tail, the max_len stop and mocr_decode_logits are untouched.
 *   Automata are per ROW: a batch may mix rows under different automata and rows under none, and the scheduler still merges
 *     requests.  A row with MOCR_AUTOMATON_NONE gives ids, lengths, scores, alternatives and positions bit-identical to the
 *     same row of a batch of the same mode and size in which nobody brings an automaton - also inside a batch with automaton
 *     rows.  A batch in which nobody brings an automaton launches exactly what it launched before.  A row under the universal
 *     automaton - one accepting state with a self-loop on every token except EOS - is bit-identical to a
 *     MOCR_AUTOMATON_NONE row.
 *   How: the rows' effective sets are the per-row masks of the no-repeat n-grams; the token kernel (profile names
 *     dec_token*_am) looks the stored token up among the old state's edges, block-wide, and rebuilds the row's mask from the
 *     new state's edges.  The tables live in one device arena allocated at full capacity by the first mocr_automaton_create
 *     (about 37 MiB; capacity is bounded by edges, not by states x 768 B, so a dictionary-sized trie fits); the rows' states
 *     (12 B a row and lane) are allocated by the first batch that brings an automaton.
 *   Beam search: the *_beam, *_beam_tokens and *_beam_positions entry points take no automaton; the *_beam_automaton twins do,
 *     under the rule of the section "beam search under a token automaton" below.
 *
 * ---- soft token automata (glossary boosts; transformers' generate(sequence_bias=...)) ----
 *   mocr_automaton_desc has two nullable trailing fields, guarded by struct_size: a caller that passes the struct without them,
 *   or nulls, gets the automaton described above.  An automaton that brings either array is SOFT.
 *     edge_weight float32 [n_edges]: finite (NaN or +-inf: MOCR_ERR_ARG); null = all 0.
 *     default_next int32 [n_states]: each in [0, n_states) or -1; null = all -1.
 *   A state s with default_next[s] >= 0 is OPEN: A(s) = every non-EOS token, plus EOS iff s accepts, and a stored non-EOS token
 *     without an edge moves the row to default_next[s].  A state with -1 is closed, as above: A(s) = its edge tokens, no edge
 *     = MOCR_STATE_DEAD.  One automaton may mix open and closed states.  EOS is still never an edge token.
 *   A default_next value may carry the bit MOCR_DEFAULT_FALLBACK (d | MOCR_DEFAULT_FALLBACK, d in [0, n_states)): then a
 *     token without an edge in s is walked from d - the row moves to the target of d's edge on that token if d has one, and to
 *     d otherwise (one level: d's own default is not followed).  Nothing else changes: s is open, and only s's own edges weigh.
 *     It is what keeps an Aho-Corasick automaton smaller: a state need not repeat the root's zero-weight edges.  It still keeps
 *     every WEIGHTED edge it inherits along its fail chain, because the LM head reads a state's own edges only: 8,000 random
 *     names over 200 tokens take 23,329 states and 866,750 edges (about 37 a state, 21 % of MOCR_MAX_AUTOMATON_EDGES) instead
 *     of 4,665,800.
 *   At the step that chooses ids[L] in state s, the logit of token t is logit(t) + edge_weight(s, t) where s has an edge on t,
 *     and the plain logit otherwise; the add is in fp32.  Everything the step derives is computed from these logits, exactly as
 *     masked columns count as -inf: the arg-max over the effective set (equal values: the lowest id), the token scores and the
 *     four alternatives, renormalised over that set, and the value a forced prefix token scores.  The effective set is A(s) AND
 *     the token set, minus the n-gram bans; the dead-end rule stays; forced prefix tokens walk default edges like emitted ones.
 *   Bit identity, as far as the caller can observe: a soft row under one accepting open state with default_next = 0 and no
 *     edges equals a MOCR_AUTOMATON_NONE row; a hard automaton created with an all-zero edge_weight equals the same automaton
 *     created without one; rows of a soft batch under a hard automaton or under none keep their results; a batch in which no
 *     row brings a soft automaton launches exactly what it launched before.
 *   How: the fused LM head's SOFT form (profile name gemm_dec_vocab_sw) adds a row's state's edge weights to the fp32 tile in
 *     LDS before it reduces it; on the slab paths the token kernel's SOFT form (dec_token*_sw) adds them to the summed logits.
 *     The arena grows by edge_weight (2^22 floats) and default_next (2^20 ints), 20 MiB, allocated at full capacity by the first
 *     create of a soft automaton and pre-filled with 0 / -1 for every automaton that exists or comes later.
 *   Beam search: a bias inside a beam's score is a different rule, not this one - the section "beam search under soft token
 *     automata" below, through the *_beam_soft entry points.  The *_beam_automaton entry points refuse a soft handle with
 *     MOCR_ERR_ARG before any work.
 *   Out of scope: weights on EOS, non-finite weights (a ban is a token set). */
#define MOCR_MAX_AUTOMATA          256
#define MOCR_MAX_AUTOMATON_STATES  (1 << 20)    /* over all automata of an engine */
#define MOCR_MAX_AUTOMATON_EDGES   (1 << 22)
#define MOCR_DEFAULT_FALLBACK      (1 << 30)    /* a bit of a default_next value: walk the token from the default state */
#define MOCR_AUTOMATON_NONE        0
enum { MOCR_STATE_NONE = -1, MOCR_STATE_DEAD = -2 };
typedef struct mocr_automaton_desc {
    int32_t struct_size;            /* sizeof(mocr_automaton_desc) */
    int32_t n_states;
    const int32_t* edge_begin;      /* [n_states + 1], edge_begin[0] = 0, monotone */
    const int32_t* edge_token;      /* [edge_begin[n_states]] */
    const int32_t* edge_next;       /* [edge_begin[n_states]], each in [0, n_states) */
    const uint8_t* accepting;       /* [n_states] */
    const float* edge_weight;       /* nullable: [edge_begin[n_states]], finite (soft token automata) */
    const int32_t* default_next;    /* nullable: [n_states], each in [0, n_states) (| MOCR_DEFAULT_FALLBACK) or -1 */
} mocr_automaton_desc;
/* A new automaton; *out_handle >= 1.  Automata are immutable and live until mocr_destroy; the arrays are copied before the
 * call returns.  Thread-safe.  MOCR_ERR_ARG: a null or short struct, n_states < 1; edge_begin[0] != 0 or edge_begin not
 * monotone; a token outside [0, vocab) or equal to EOS; tokens of a state not strictly ascending; edge_next outside
 * [0, n_states); a non-finite edge_weight; default_next outside [0, n_states) and not -1; a table or the handle list full.
 * MOCR_ERR_STATE before mocr_commit_weights. */
int mocr_automaton_create(mocr_engine* e, const mocr_automaton_desc* desc, int32_t* out_handle);
int mocr_automaton_count(mocr_engine* e);
/* Device bytes the automata hold: the arena (its soft part from the first soft create on) plus the lanes' row states (and, 4 B a row more, the hypothesis states of a lane
 * that has run a beam batch under an automaton); 0 until the first create / first automaton batch. */
int64_t mocr_automaton_state_bytes(mocr_engine* e);
/* The *_automaton entry points: the *_shared twins plus `automata`, a HOST int32 array [n_rows] of handles (null: every row
 * MOCR_AUTOMATON_NONE; copied before the call returns), and out_state int32 [n_rows] (nullable; host, or device for the device
 * twin): the state the row was in after its last non-EOS token, in its automaton's own numbering; MOCR_STATE_NONE for a row
 * without an automaton or of a sliver region, MOCR_STATE_DEAD for a dead row.  With both null they ARE the shared calls.  An
 * unknown handle is MOCR_ERR_ARG before any work. */
int mocr_recognize_images_automaton(mocr_engine* e, const mocr_image* images, int32_t n_images, int32_t n_rows, const int32_t* source,
                                    int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                    const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                    const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, int32_t* out_state);
int mocr_recognize_regions_automaton(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                     int32_t n_regions, int32_t n_rows, const int32_t* source, int32_t* out_ids, int32_t* out_len,
                                     float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                     float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld,
                                     const int32_t* automata, int32_t* out_state);
int mocr_recognize_device_automaton(mocr_engine* e, const void* d_gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                    void* d_out_ids, void* d_out_len, void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp,
                                    const int32_t* sets, const int32_t* ngram, void* d_out_pos, const int32_t* prefix,
                                    const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, void* d_out_state);
int mocr_recognize_gray_host_automaton(mocr_engine* e, const uint8_t* gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                       int32_t max_len_override, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                       float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos,
                                       const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata,
                                       int32_t* out_state);

/* ---- repetition penalty (transformers' generate(repetition_penalty=p) under greedy search) --------------------------------
 * The *_penalty entry points: the *_automaton twins plus `penalty`, a HOST float32 array [n_rows] with one p per row (null:
 * every row 1 - then the call IS the *_automaton call).  Each p is finite and > 0 (anything else: MOCR_ERR_ARG before any
 * work); p < 1 rewards repeats and is allowed, as in transformers; p = 1 is off.
 *   The rule is RepetitionPenaltyLogitsProcessor's, per row.  At the step that chooses ids[t + 1], `seen` is the set of ids at
 *     positions 0 .. t of the row: the start token, forced prefix tokens and chosen tokens.  For every token c in `seen`, with v
 *     the fp32 logit: v' = v < 0 ? v * p : v / p - an IEEE fp32 multiply or divide, never a reciprocal; v == 0 divides.
 *   Order with the other processors is transformers': sequence_bias (a soft automaton's edge weight) first, then the penalty,
 *     then the bans - v is (acc + edge weight) + bias, and the token sets, n-gram bans and automaton sets turn a column into
 *     -inf afterwards.
 *   Everything the step derives from the logits sees v': the arg-max (equal values: the lowest id), the token scores - the
 *     log_softmax of the penalised, masked row -, the four alternatives, and the value a forced prefix token scores.  Prefix
 *     steps are causal: step t sees the tokens before it.  mocr_decode_logits stays raw.
 *   Bit identity: v * 1 and v / 1 are exact, so a row with p = 1 beside penalised rows returns the ids, scores and
 *     alternatives it returns in a batch without the array; a batch in which every p is 1 launches exactly what it launched.
 *   How: by ROW like ids, seen_mask uint32 [rows][192] and penalty_of_row float [rows] (772 B a row and lane, allocated by the
 *     first batch with a p != 1; the same batch allocates the automaton arena and its soft part if no automaton has yet).  The
 *     fused LM head's PEN form (profile name gemm_dec_vocab_rp) and the token kernel's (dec_token*_rp) are SOFT forms too: rows
 *     without an automaton are in MOCR_STATE_NONE and add nothing.
 *   Out of scope: beam search - a beam request cannot carry a penalty (under beams transformers penalises log-probabilities). */
int mocr_recognize_images_penalty(mocr_engine* e, const mocr_image* images, int32_t n_images, int32_t n_rows, const int32_t* source,
                                  int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                  const int32_t* sets, const int32_t* ngram, float* out_pos, const int32_t* prefix,
                                  const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, int32_t* out_state,
                                  const float* penalty);
int mocr_recognize_regions_penalty(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                   int32_t n_regions, int32_t n_rows, const int32_t* source, int32_t* out_ids, int32_t* out_len,
                                   float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets, const int32_t* ngram,
                                   float* out_pos, const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld,
                                   const int32_t* automata, int32_t* out_state, const float* penalty);
int mocr_recognize_device_penalty(mocr_engine* e, const void* d_gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                  void* d_out_ids, void* d_out_len, void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp,
                                  const int32_t* sets, const int32_t* ngram, void* d_out_pos, const int32_t* prefix,
                                  const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata, void* d_out_state,
                                  const float* penalty);
int mocr_recognize_gray_host_penalty(mocr_engine* e, const uint8_t* gray, int32_t n_planes, int32_t n_rows, const int32_t* source,
                                     int32_t max_len_override, int32_t* out_ids, int32_t* out_len, float* out_logp, int32_t* out_alt_ids,
                                     float* out_alt_logp, const int32_t* sets, const int32_t* ngram, float* out_pos,
                                     const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld, const int32_t* automata,
                                     int32_t* out_state, const float* penalty);

/* Preprocessing only (test hook): out_gray [n, image_size, image_size] uint8 (host) = the plane the encoder sees
 * in each of its three equal input channels before the 1/255 and (x - 0.5)/0.5 scaling. */
int mocr_preprocess(mocr_engine* e, const mocr_image* images, int32_t n, uint8_t* out_gray);

/* THE HOT PATH (device buffers, asynchronous): submits one batch.  d_gray is a device pointer to
 * n contiguous image_size x image_size uint8 luminance planes, d_out_ids / d_out_len device
 * pointers ([n,max_len] / [n] int32), n <= max_batch; all three must stay valid until
 * mocr_synchronize() returns.  Batches submitted back to back run concurrently on the engine's
 * lanes; mocr_synchronize() schedules every submitted batch to completion (greedy steps in
 * chunks, stopping a batch once all of its rows have emitted EOS) and waits for the GPU. */
int mocr_recognize_device(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len);
/* mocr_recognize_device plus d_out_logp, a device pointer to [n, max_len] float32 (token scores, see above; nullable). */
int mocr_recognize_device_scored(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len, void* d_out_logp);
/* ... plus d_out_alt_ids int32 / d_out_alt_logp float32, device pointers to [n, max_len, MOCR_ALTERNATIVES] (token
 * alternatives, see above; both null or both set). */
int mocr_recognize_device_alts(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len, void* d_out_logp,
                               void* d_out_alt_ids, void* d_out_alt_logp);
/* ... plus `sets`, a HOST array of n token-set handles (token constraints, see above; nullable). */
int mocr_recognize_device_constrained(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len,
                                      void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets);
/* ... plus `ngram`, a HOST array of n no-repeat n-gram sizes (no-repeat n-grams, see above; nullable). */
int mocr_recognize_device_norepeat(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len,
                                   void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets,
                                   const int32_t* ngram);
/* ... plus d_out_pos, a device pointer to [n, max_len, MOCR_POSITION_FIELDS] float32 (token positions, see above; nullable). */
int mocr_recognize_device_positions(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len,
                                    void* d_out_logp, void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets,
                                    const int32_t* ngram, void* d_out_pos);
/* ... plus prefix / prefix_len / prefix_ld, HOST arrays (forced prefixes, see above; both null or both set). */
int mocr_recognize_device_prefix(mocr_engine* e, const void* d_gray, int32_t n, void* d_out_ids, void* d_out_len, void* d_out_logp,
                                 void* d_out_alt_ids, void* d_out_alt_logp, const int32_t* sets, const int32_t* ngram, void* d_out_pos,
                                 const int32_t* prefix, const int32_t* prefix_len, int32_t prefix_ld);
/* generate(max_length=...) of every batch submitted from now on, whatever the entry point (2 <= max_len <= the
 * engine's max_len; rows are still max_len wide; mocr_recognize_gray_host's own argument overrides it).  The reference always calls generate with 300; a speech bubble is
 * typically ~32 tokens (SURVEY.md §8d reports both regimes). */
int mocr_set_generate_max_length(mocr_engine* e, int32_t max_len);
int mocr_synchronize(mocr_engine* e);
/* The hipStream_t of lane 0 (the stream the test hooks and single-lane engines launch on). */
void* mocr_stream(mocr_engine* e);

/* ---- test hooks (fp32 out; used by tests/ and __graft_entry__.smoke()) -------------------- */
/* Encoder only: h_out [n, 197, hidden] float32 (final LayerNorm output). */
int mocr_encode(mocr_engine* e, const void* d_gray, int32_t n, float* h_out);
/* Teacher-forced decode: inputs forced_ids [n, T] (forced_ids[:,0] must be start_id);
 * h_logits [n, T, vocab] float32 = logits after consuming forced_ids[:, :t+1]. */
int mocr_decode_logits(mocr_engine* e, const void* d_gray, int32_t n, const int32_t* forced_ids,
                       int32_t T, float* h_logits);
/* Greedy decode limited to max_len_override tokens (<= max_len); host outputs. */
int mocr_recognize_gray_host(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                             int32_t* out_ids, int32_t* out_len);
int mocr_recognize_gray_host_scored(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                    int32_t* out_ids, int32_t* out_len, float* out_logp);   /* + token scores (nullable) */
int mocr_recognize_gray_host_alts(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                  int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp);   /* + token alternatives */
int mocr_recognize_gray_host_constrained(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                         int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                         const int32_t* sets);   /* + token constraints */
int mocr_recognize_gray_host_norepeat(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                      int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                      const int32_t* sets, const int32_t* ngram);   /* + no-repeat n-grams */

int mocr_recognize_gray_host_positions(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                       int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp,
                                       const int32_t* sets, const int32_t* ngram, float* out_pos);   /* + token positions */

int mocr_recognize_gray_host_prefix(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override, int32_t* out_ids,
                                    int32_t* out_len, float* out_logp, int32_t* out_alt_ids, float* out_alt_logp, const int32_t* sets,
                                    const int32_t* ngram, float* out_pos, const int32_t* prefix, const int32_t* prefix_len,
                                    int32_t prefix_ld);   /* + forced prefixes */

/* Single operators on device buffers of the engine's dtype (kernel unit tests). */
int mocr_op_gemm(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, void* d_out,
                 const float* d_resid, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                 int32_t tile, int32_t split_k);
int mocr_op_layernorm(mocr_engine* e, const float* d_x, const float* d_gamma, const float* d_beta,
                      void* d_out, int32_t M);
/* bf16 engines: the persistent encoder GEMM (tile 4096 / 4097 / 4099 / 4100) with the LayerNorm folded in.
 * epilogue 3 (bias + residual, fp32 out): also writes d_xb [M,N] bf16 = the output rows and d_part [M,4,2] float32 = each
 * row's (sum, sum of squares) per 256-column slice.  epilogue 1 / 2 (bias / bias + GELU, bf16 out): dA = the rows x as bf16,
 * dW = bf16(W o gamma), d_bias = b + W beta, d_csum [N] = column sums of dW, d_part = the statistics of the fp32 rows:
 * out = LN(x) W^T + b.  mocr_op_ln_prep: d_x [M,768] float32 -> d_xb bf16 + d_part (partial 0 = the row's sums). */
int mocr_op_gemm_ln(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, void* d_out,
                    const float* d_resid, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t tile,
                    float* d_part, const float* d_csum, void* d_xb);
int mocr_op_ln_prep(mocr_engine* e, const float* d_x, void* d_xb, float* d_part, int32_t M);
int mocr_op_enc_attention(mocr_engine* e, const void* d_qkv, void* d_ctx, int32_t n, int32_t impl);
/* The encoder's front end, launched as the encoder launches it: d_gray uint8 [n,224,224] -> d_patches [round_up(n*196, 128), 256]
 * of the engine's dtype (rows n*196 .. are left alone) -> d_x float32 [n*197, 768]: row b*197 = cls + pos[0], row b*197 + 1 + p =
 * patch p of crop b times the channel-summed patch weight + bias + pos[1 + p].  tile: the patch embedding's GEMM tile, 64 or 128;
 * 0 = the encoder's own choice for n crops (mocr_encoder_plan).  n <= max_batch. */
int mocr_op_embed(mocr_engine* e, const void* d_gray, int32_t n, int32_t tile, void* d_patches, float* d_x);
/* What finishes an encoder GEMM split over K: d_x [M,768] float32 += d_bias + the nslab slabs d_slabs + k * slab_stride (floats,
 * a multiple of 4, >= M * 768), summed in the order k = 0, 1, ..., in place; d_out [M,768] of the engine's dtype = LayerNorm(d_x). */
int mocr_op_layernorm_slab(mocr_engine* e, float* d_x, const float* d_slabs, int32_t nslab, int64_t slab_stride,
                           const float* d_bias, const float* d_gamma, const float* d_beta, void* d_out, int32_t M);
/* What the encoder decides from the number of crops n <= max_batch (test hook; the decisions also depend on the engine's dtype,
 * flags, compute units and max_batch): out = { patch-embedding tile, tile codes of QKV / O-proj / FC1 / FC2 (64, 128, 4096),
 * K slices of O-proj, K slices of FC2 (1 = not split; the LayerNorm behind a split GEMM adds that many slabs), 1 if the
 * LayerNorms are folded into the GEMMs, blocks per (crop, head) of the attention, attention kernel (0 VALU, 1 matrix cores) }. */
int mocr_encoder_plan(mocr_engine* e, int32_t n, int32_t out[10]);
/* The rest of that plan: out = { N-tiles per column group of the tile order of QKV, of FC1 } for n crops - 9 / 12 on the 128 x 128
 * kernel, 6 / 6 on the persistent one (column groups 6 + 3 and 6 + 6 of 256-column tiles). */
int mocr_encoder_groups(mocr_engine* e, int32_t n, int32_t out[2]);
/* What a greedy decode step of `rows` rows decides on this engine (test hook; computed by the helpers the step launches
 * through, nothing is launched).  regime_rows = the rows the batch started with (0 = rows): after a compaction the split over
 * K follows the regime, the tile and the ring depth follow the rows that are left.  rows need not fit max_batch.  out =
 *   [0]  path: 0 small-batch (bf16, <= 32 regime rows, not latent), 1 classic attention, 2 latent attention (bf16, regime rows
 *        above the engine's own switch: min(256, max_batch), 0 with MOCR_FLAG_LATENT_ALWAYS, never with
 *        MOCR_FLAG_CLASSIC_ATTENTION) - the path fields [0], [18] .. [22] use THIS engine's switch
 *   [1]  regime tile: 128 from 1024 regime rows, else 64 (the split is chosen for it)     [2] launch tile: the same rule on rows
 *   [3 + 3 g], [4 + 3 g], [5 + 3 g] for g = 0 QKV [2304 x 768], 1 the 768 x 768 projections, 2 FC1 [3072 x 768], 3 FC2
 *        [768 x 3072], 4 vocabulary [vocab x 768]: K slices (1 = not split), ring slots of the launch (2 or 4: 4 iff rows <
 *        1280, >= 4 K-tiles of 128 bytes per K slice and M-tiles x N-tiles x slices <= compute units) and the epilogue launched:
 *        0 fp32 slabs; FC1 2 = bias + GELU fused (its split is 1); vocabulary 6 = the fused LM head (split 1, no
 *        MOCR_FLAG_NO_FUSED_ARGMAX; a scored / constrained batch launches that head's own form of it, a logits or beam request
 *        the slabs).  These fifteen say how gemm_kernel is launched for the shape at these rows whether or not the path
 *        launches it; they depend on the dtype, the compute units and the flags, not on max_batch
 *   [18] 1 if the step launches QKV as a tile GEMM (classic path; the latent path projects the queries in its own block and the
 *        small-batch path launches none of the five as a tile GEMM)
 *   [19] latent path: 1 if q and Qt come from the fused query kernel (from 257 regime rows)   [20] its rows per block (64 up to
 *        1280 rows, else 128; 0 when not fused)   [21] the Qt GEMM's tile on the two-launch path (128 from 1024 regime rows, else
 *        64; 0 when fused or not latent)
 *   [22] classic and small-batch attention: 1 = non-temporal K/V loads (from 128 regime rows)
 *   [23] steps per graph replay: 2 up to 16 rows, 4 up to 128, else 8
 *   [24] the rows a batch of `rows` decodes on: rows rounded up to 1 (<= 8), 8 (<= 64), 32 (<= 256), 64 (<= 1024) or 256,
 *        at most max_batch. */
#define MOCR_DECODE_PLAN_FIELDS 25
int mocr_decode_plan(mocr_engine* e, int32_t rows, int32_t regime_rows, int32_t out[MOCR_DECODE_PLAN_FIELDS]);
/* mocr_op_gemm on the 64 / 128 tile kernel with the operands a caller of the engine sets itself: the decode step's slabs lie
 * round_up(max_batch, 128) * N floats apart, the encoder walks QKV / FC1 in column groups.  Through the same launch, so the
 * ring depth is the one the step gets at M rows.  Refuses what mocr_op_gemm refuses, a tile code other than 64 / 128, rows
 * that are not 16-byte aligned and a slab stride that cannot hold a slab.  A holds M rounded up to the tile rows. */
typedef struct mocr_gemm_args {
    int32_t struct_size;        /* sizeof(mocr_gemm_args) */
    int32_t M, N, K;
    int32_t epilogue;           /* 0 slabs, 1 bias, 2 bias + GELU, 3 bias + residual (fp32 out), 5 bias (fp32 out) */
    int32_t tile;               /* 64 or 128 */
    int32_t split_k;            /* K slices (> 1 with epilogue 0 only) */
    int32_t lda;                /* elements between two rows of A (0 = K) */
    int32_t ldo;                /* elements between two rows of out and of resid (0 = N) */
    int32_t group_n;            /* N-tiles per column group of the tile order (0 = one group) */
    int64_t slab_stride;        /* epilogue 0: floats between two K slices' slabs (0 = M * ldo) */
    const void* A;
    const void* W;              /* [N][K] */
    const float* bias;          /* [N]; unused by epilogue 0 */
    void* out;
    const float* resid;         /* epilogue 3 */
} mocr_gemm_args;
int mocr_op_gemm_args(mocr_engine* e, const mocr_gemm_args* a);
/* The calling thread's last gemm_kernel launch (any hook that runs a 64 / 128 tile GEMM, the fused LM heads included):
 * out = { tile, ring slots, blocks in the grid, K slices }. */
int mocr_last_tile_launch(mocr_engine* e, int32_t out[4]);
/* bf16 engines: the persistent encoder GEMM launched as the encoder launches a layer GEMM - dense rows, out = A W^T + bias
 * through the epilogue, the tile order in column groups of group_n N-tiles, the LayerNorm fold operands of mocr_op_gemm_ln when
 * ln_part is set (csum and xb come with it only).  Refuses what the engine's own GEMM call and the kernel's launch refuse, with
 * their messages.  Tile-list codes stage whole 256-row tiles of A (A holds M rounded up to 256 rows); the strip codes read no row
 * behind M and need M >= 256. */
typedef struct mocr_gemm_pers_args {
    int32_t struct_size;        /* sizeof(mocr_gemm_pers_args) */
    int32_t M;
    int32_t N;                  /* a multiple of 256 */
    int32_t K;                  /* a multiple of 64, >= 128 */
    int32_t epilogue;           /* 1 bias, 2 bias + GELU (bf16 out), 3 bias + residual (fp32 out) */
    int32_t tile;               /* 4096 the product's choice of schedule, 4097 the tile list on 8 blocks, 4099 strips, 4100 strips on 8 blocks */
    int32_t group_n;            /* N-tiles per column group of the tile order (0 = one group); the strip schedule has no tile order */
    const void* A;              /* [M][K] bf16 */
    const void* W;              /* [N][K] bf16 */
    const float* bias;          /* [N] */
    void* out;                  /* [M][N] */
    const float* resid;         /* epilogue 3: [M][N], may be out */
    float* ln_part;             /* [M][4][2] or null: written by epilogue 3, read by 1 and 2 */
    const float* csum;          /* [N], epilogues 1 and 2 with ln_part */
    void* xb;                   /* [M][N] bf16, epilogue 3 with ln_part */
} mocr_gemm_pers_args;
int mocr_op_gemm_pers(mocr_engine* e, const mocr_gemm_pers_args* a);
/* The calling thread's last launch of the persistent kernel (any hook that runs it): out = { blocks in the grid, 1 if the strip
 * schedule ran (0: the tile list), tiles (M-tiles x N-tiles of 256 x 256), group_n as the kernel was given it }. */
int mocr_last_pers_launch(mocr_engine* e, int32_t out[4]);
/* Latent decode attention (bf16 engines): d_qt [n,16,768], keys d_x with x_batch_stride elements between
 * sequences, context length len for every row; d_out [n,16,768] = softmax(qt . x^T) x per head. */
int mocr_op_latent_attention(mocr_engine* e, const void* d_qt, const void* d_x, void* d_out, int32_t n, int32_t len,
                             int64_t x_batch_stride);

/* fp8 attention (MOCR_FLAG_FP8_ATTENTION) operators: d_x bf16 [n_elems] -> d_x8 e4m3 [n_elems] = e4m3(x * inv_sx);
 * and the latent attention on e4m3 key rows (768 B per key, x = x8 * sx): d_qt [n,16,768] bf16, d_out [n,16,768] bf16. */
int mocr_op_quant_fp8(mocr_engine* e, const void* d_x, void* d_x8, int64_t n_elems, float inv_sx);
int mocr_op_latent_attention_fp8(mocr_engine* e, const void* d_qt, const void* d_x8, void* d_out, int32_t n, int32_t len,
                                 int64_t x_batch_stride_bytes, float sx);

/* Fused query path of the latent attention (bf16 engines): d_x [rows_pad,768] bf16 (rows_pad = n rounded up to 128),
 * d_wq [768,768] bf16, d_bq [768] f32, d_wkT [768,768] bf16 (row n, column 64h+k = Wk_h[k][n]/8), d_qt [rows_pad,16,768] bf16:
 * d_qt[m][h] = bf16(x[m] . Wq_h^T + bq_h) . wkT_h   for the 12 heads. */
int mocr_op_qqt(mocr_engine* e, const void* d_x, const void* d_wq, const float* d_bq, const void* d_wkT, void* d_qt, int32_t n);

/* Decode-step operators (kernel unit tests).  Each launches through the helper the decode step itself uses - the kernel
 * variant it picks included - on the caller's device buffers; T = the engine's dtype, slab inputs are split-K partial sums
 * [nslab][rows][N] fp32, and max_len / vocab / hidden are the engine's.
 * Classic decode attention.  self != 0: d_slabs [nslab][n][2304] (q | k | v), d_bias [2304], d_k / d_v the K / V cache
 * [rows][heads][max_len][64] T; slot s attends to row rowmap[s] (identity when d_rowmap is null): the cached positions
 * 0 .. step[s] - 1 and its new key / value, which are appended at position step[s].  approx_len picks the kernel variant and
 * must bound every step[s] + 1.  self == 0: d_slabs [nslab][n][768], d_bias [768], d_k = a cross K/V block [rows][197][NCKV]
 * (NCKV = 2 x hidden x decoder layers; `layer` selects the K | V column pair), d_v and d_step unused.  d_ctx [n][768] T.
 * nt: the K/V load policy (0 cached, 1 non-temporal), -1 = the decode step's choice for n rows. */
int mocr_op_dec_attn(mocr_engine* e, int32_t self, const float* d_slabs, int32_t nslab, const float* d_bias, void* d_k, void* d_v,
                     int32_t layer, const int32_t* d_step, const int32_t* d_rowmap, void* d_ctx, int32_t n, int32_t approx_len,
                     int32_t nt);
/* out = LayerNorm([gelu](sum of the slabs + bias) [+ d_resid]) on rows of 768: d_out_f32 [rows][768] (nullable), d_out_t
 * [rows][768] T.  d_cache (nullable): the row is also written to row rowmap[s], position step[s] of d_cache [..][max_len][768]:
 * as T, or (cache_fp8) as the e4m3 bytes of out * inv_sx. */
int mocr_op_dec_add_ln(mocr_engine* e, const float* d_slabs, int32_t nslab, const float* d_bias, const float* d_resid,
                       const float* d_gamma, const float* d_beta, int32_t gelu, float* d_out_f32, void* d_out_t, int32_t rows,
                       void* d_cache, int32_t cache_fp8, float inv_sx, const int32_t* d_step, const int32_t* d_rowmap);
/* d_out [rows][N] T = gelu(sum of the slabs + d_bias). */
int mocr_op_dec_bias_gelu(mocr_engine* e, const float* d_slabs, int32_t nslab, const float* d_bias, void* d_out, int32_t rows,
                          int32_t N);
/* The token step (argmax, finish rules, next input embedding + LayerNorm from the engine's embedding weights).  Buffers indexed
 * by decode slot: slabs, cand_*, forced, step, rowmap, x_f32, x_t; by row: ids, finished, len, cache. */
typedef struct mocr_token_args {
    int32_t struct_size;        /* sizeof(mocr_token_args) */
    int32_t first;              /* 1: the start step (start token, rowmap = identity, rows >= n_real born finished) */
    int32_t n;                  /* decode slots */
    int32_t nslab;              /* slab path: slabs [nslab][n][vocab] */
    const float* slabs;
    const float* vbias;         /* slab path: LM-head bias [vocab]; null = the engine's */
    const float* cand_val;      /* candidate path (ncand > 0): [n][ncand] per-tile maxima and their columns */
    const int32_t* cand_idx;
    int32_t ncand;
    int32_t forced_T;
    const int32_t* forced;      /* nullable: [n][forced_T] ids that override the argmax */
    int32_t* ids;               /* [rows][ids_ld] */
    int32_t* step;              /* [n] */
    int32_t* finished;          /* [rows] */
    int32_t* len;               /* [rows] */
    int32_t* n_unfinished;      /* [1] */
    int32_t* rowmap;            /* [n] */
    int32_t ids_ld;
    int32_t max_len;            /* generate(max_length) */
    int32_t n_real;
    int32_t cache_fp8;          /* cache holds e4m3 bytes of x * inv_sx */
    float* x_f32;               /* [n][768] */
    void* x_t;                  /* [n][768] T */
    void* cache;                /* nullable: [rows][max_len][768], position step + 1 is written */
    float inv_sx;
} mocr_token_args;
int mocr_op_dec_token(mocr_engine* e, const mocr_token_args* a);
/* The scored token step (token scores): the same launch with d_scores [rows][ids_ld] float32, indexed by row like ids:
 * d_scores[rowmap[s]][step[s] + 1] = -log(sum_j exp(logit_j - max)) of slot s, 0 when the row is finished.  Candidate path:
 * d_cand_sum [n][ncand] = the tiles' sums of exp(logit - cand_val) (mocr_op_gemm_argmax_lse); slab path: d_cand_sum unused.
 * Not with first or forced ids.  d_scores = NULL is mocr_op_dec_token.  Rows without a finite logit score NaN. */
int mocr_op_dec_token_scored(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores);
/* The token step with alternatives (token alternatives): the scored launch plus d_alt_ids int32 / d_alt_logp float32
 * [rows][ids_ld][4], indexed by row like ids: [rowmap[s]][step[s] + 1][k] = the token with the k-th largest logit of slot s
 * and (logit_k - max) - log(sum_j exp(logit_j - max)); -1 / 0 when the row is finished.  Candidate path: d_top_val / d_top_idx
 * [n][ncand][4] = the tiles' four best (mocr_op_gemm_topk); slab path: unused.  Needs d_scores; restrictions as for the scored
 * step.  d_alt_ids = d_alt_logp = NULL is mocr_op_dec_token_scored. */
int mocr_op_dec_token_topk(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                           const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp);
/* The token step under token sets (token constraints): d_tok_mask uint32 [sets][vocab / 32] (bit v of a set's row = token v is
 * allowed; the caller keeps EOS in every set) and d_set_of_row int32 [rows], the set of every ROW (slot s decodes row
 * rowmap[s] under set d_set_of_row[rowmap[s]]).  Runs the ids, scored or alternatives form by which outputs are non-null, as
 * mocr_op_dec_token_topk does.  Candidate path: the candidates come from mocr_op_gemm_argmax_masked; slab path: the kernel
 * masks the summed logits itself.  Not with first or forced ids.  d_tok_mask = d_set_of_row = NULL is mocr_op_dec_token_topk. */
int mocr_op_dec_token_masked(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                             const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                             const uint32_t* d_tok_mask, const int32_t* d_set_of_row);
/* The token step with no-repeat n-grams: mocr_op_dec_token_masked plus d_row_mask uint32 [rows][vocab / 32] (in / out: the
 * effective set of every ROW's next step), d_base_mask uint32 [sets][vocab / 32] with d_base_set_of_row int32 [rows] (the
 * rows' token sets, which a rebuilt mask starts from) and d_ngram_of_row int32 [rows] (the rows' sizes, 0 = off).  The step
 * itself is the masked one on d_tok_mask / d_set_of_row - the engine passes d_tok_mask = d_row_mask and d_set_of_row = 0, 1,
 * 2, ... so that a row reads its own mask; then, for every unfinished row with n > 0, row_mask[row] = its base set minus the
 * bans of the step that follows the token just stored (the rule above, on the row's ids).  Other rows' masks are left as
 * they are.  The four new pointers all NULL is mocr_op_dec_token_masked. */
int mocr_op_dec_token_ngram(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                            const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                            const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                            const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row);
/* The token step with forced prefixes: mocr_op_dec_token_ngram plus d_prefix int32 [rows][prefix_ld] and d_prefix_len int32
 * [rows], by ROW, and d_tgt_val float32 [n], by SLOT (candidate path: mocr_op_gemm_argmax_target's; slab path: unused).  Slot s
 * with step[s] < d_prefix_len[rowmap[s]] stores, finishes on and embeds d_prefix[row][step[s]] and scores it by the rule above.
 * Needs d_scores and d_tok_mask.  d_prefix = d_prefix_len = NULL is mocr_op_dec_token_ngram. */
int mocr_op_dec_token_prefix(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                             const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                             const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                             const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                             const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val);
/* The start of a batch with no-repeat n-grams: d_row_mask[row] = d_base_mask[d_base_set_of_row[row]] for rows [0, rows), with
 * the start token's bit cleared where d_ngram_of_row[row] == 1 (the first generated token already sees L = 1). */
int mocr_op_ngram_init(mocr_engine* e, uint32_t* d_row_mask, const uint32_t* d_base_mask, const int32_t* d_base_set_of_row,
                       const int32_t* d_ngram_of_row, int32_t rows);
/* The token step with token automata: mocr_op_dec_token_prefix plus the tables in CSR form over GLOBAL state numbers -
 * d_edge_begin int32 [states + 1], d_edge_token / d_edge_next int32 [edges], d_accepting uint8 [states] - and by ROW
 * d_aut_base_of_row int32 [rows] (the row's start state, -1: no automaton) and d_aut_state int32 [rows] (in / out: the state
 * the row is in, MOCR_STATE_DEAD allowed).  A row that was unfinished before the step and brings an automaton walks its state
 * with the stored token and, if still unfinished, gets row_mask[row] rebuilt by the rule of the token automata section; a row
 * without one takes mocr_op_dec_token_prefix's path.  Needs d_row_mask.  The six new pointers all NULL is that call. */
int mocr_op_dec_token_automaton(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                                const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                                const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                                const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                                const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val,
                                const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                                const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state);
/* The token step with soft token automata: mocr_op_dec_token_automaton plus d_edge_weight float32 [edges] and d_default_next
 * int32 [states] (global numbers, with MOCR_DEFAULT_FALLBACK where set; -1: closed), both or neither.  Slab path: the weights of the row's state's edges are added to
 * the summed logits before masking; walk: no edge -> d_default_next[state], DEAD only where that is -1; rebuild: an open state
 * starts from every token, EOS by d_accepting.  Both NULL is mocr_op_dec_token_automaton. */
int mocr_op_dec_token_soft(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                           const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                           const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                           const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                           const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val,
                           const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                           const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state,
                           const float* d_edge_weight, const int32_t* d_default_next);
/* The token step with a repetition penalty: mocr_op_dec_token_soft plus d_seen_mask uint32 [rows][192] and d_penalty_of_row
 * float32 [rows], both by ROW and both or neither; they come with the four per-row mask arrays (d_row_mask ...).  Slab path:
 * the thread's logits whose bit is set are penalised after the edge weights and before the masking.  Both paths: the token
 * stored for a row that was unfinished before the step has its bit set in d_seen_mask.  Both NULL is mocr_op_dec_token_soft;
 * the eight automaton arrays may all be NULL beside them (a penalty without any automaton), and an automaton beside them
 * brings d_edge_weight and d_default_next. */
int mocr_op_dec_token_penalty(mocr_engine* e, const mocr_token_args* a, const float* d_cand_sum, float* d_scores,
                              const float* d_top_val, const int32_t* d_top_idx, int32_t* d_alt_ids, float* d_alt_logp,
                              const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint32_t* d_row_mask,
                              const uint32_t* d_base_mask, const int32_t* d_base_set_of_row, const int32_t* d_ngram_of_row,
                              const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld, const float* d_tgt_val,
                              const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                              const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state,
                              const float* d_edge_weight, const int32_t* d_default_next, uint32_t* d_seen_mask,
                              const float* d_penalty_of_row);
/* The start of a batch with a repetition penalty: d_seen_mask [rows][vocab / 32] = the start token's bit alone. */
int mocr_op_penalty_init(mocr_engine* e, uint32_t* d_seen_mask, int32_t rows);
/* The start of a batch with soft token automata: mocr_op_automaton_init, where a start state with d_default_next >= 0 is open.
 * d_default_next NULL is mocr_op_automaton_init. */
int mocr_op_automaton_init_soft(mocr_engine* e, uint32_t* d_row_mask, const uint32_t* d_base_mask, const int32_t* d_base_set_of_row,
                                const int32_t* d_ngram_of_row, int32_t rows, const int32_t* d_edge_begin, const int32_t* d_edge_token,
                                const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state,
                                const int32_t* d_default_next);
/* The start of a batch with token automata: for rows [0, rows), a row with d_aut_base_of_row[row] >= 0 gets
 * d_row_mask[row] = A(start) AND its base set, minus the start token where d_ngram_of_row[row] == 1, {EOS} if that is empty,
 * and d_aut_state[row] = its start state; any other row gets what mocr_op_ngram_init gives it and MOCR_STATE_NONE. */
int mocr_op_automaton_init(mocr_engine* e, uint32_t* d_row_mask, const uint32_t* d_base_mask, const int32_t* d_base_set_of_row,
                           const int32_t* d_ngram_of_row, int32_t rows, const int32_t* d_edge_begin, const int32_t* d_edge_token,
                           const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state);
/* The expansion of shared encodings, as a batch runs it: d_enc holds max(n_src, n_rows) rows of 197 x hidden elements of the
 * engine's dtype, its first n_src rows the encodings; d_src_of_row is a device int32 [n_rows] of indices into them.  On return
 * row r < n_rows holds what row d_src_of_row[r] held before the call (in place from the caller's view: the engine stages the
 * sources in its own workspace first); rows >= n_rows are not written.  n_src, n_rows <= max_batch; lane 0's stream. */
int mocr_op_enc_expand(mocr_engine* e, void* d_enc, const int32_t* d_src_of_row, int32_t n_src, int32_t n_rows);
/* The positions kernel (token positions), launched through the helper the deferred pass uses: d_q [rows][T][768] queries and
 * d_k [rows][197][768] keys in the engine's dtype, d_len [rows] int32 - positions 0 .. d_len[r] - 1 of row r are computed
 * (at most T), the rest written as 0.  d_out_pos [rows][T][MOCR_POSITION_FIELDS] float32; d_out_map (nullable) float32
 * [rows][T][197] = the head-mean map a.  Nothing behind a row's 197 keys is read. */
int mocr_op_attn_positions(mocr_engine* e, const void* d_q, const void* d_k, const int32_t* d_len, int32_t rows, int32_t T,
                           float* d_out_pos, float* d_out_map);
/* ... in its gathered-query form (token positions of beam hypotheses): plus d_trail, uint8 [rows][trail_ld] with
 * trail_ld >= T + 1, and K (1 .. MOCR_MAX_BEAMS; rows a multiple of it).  The query of position p of row r is read from row
 * (r / K) * K + min(d_trail[r][p + 1], K - 1), position p, of d_q; keys, lengths and outputs stay by row r.  With d_trail null
 * it is mocr_op_attn_positions. */
int mocr_op_attn_positions_gathered(mocr_engine* e, const void* d_q, const void* d_k, const int32_t* d_len, int32_t rows, int32_t T,
                                    float* d_out_pos, float* d_out_map, const uint8_t* d_trail, int32_t trail_ld, int32_t K);
/* The LM head's fused argmax GEMM (tile 64 or 128, not split): d_cand_val / d_cand_idx [M][N / tile] = per row and N-tile
 * the largest acc + bias and its column (the lowest column on a tie).  dA holds M rounded up to the tile. */
int mocr_op_gemm_argmax(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                        int32_t* d_cand_idx, int32_t M, int32_t N, int32_t K, int32_t tile);
/* The scored LM head (token scores): mocr_op_gemm_argmax plus d_cand_sum [M][N / tile] = per row and N-tile the sum over the
 * tile's columns of exp(acc + bias - d_cand_val); d_cand_val / d_cand_idx are bit-identical to mocr_op_gemm_argmax's. */
int mocr_op_gemm_argmax_lse(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                            int32_t* d_cand_idx, float* d_cand_sum, int32_t M, int32_t N, int32_t K, int32_t tile);
/* The LM head with alternatives (token alternatives): mocr_op_gemm_argmax_lse plus d_top_val / d_top_idx [M][N / tile][4] =
 * per row and N-tile the four largest acc + bias and their columns (value descending, the lower column first on a tie;
 * entry 0 = d_cand_val / d_cand_idx); the three candidate arrays are bit-identical to mocr_op_gemm_argmax_lse's. */
int mocr_op_gemm_topk(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                      int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N, int32_t K,
                      int32_t tile);
/* The LM head under token sets (token constraints): GEMM row m is decode slot m = batch row d_rowmap[m] (NULL: m), decoded
 * under set d_set_of_row[row] of d_tok_mask uint32 [sets][N / 32]; columns outside the set are left out of the max, the exp sum
 * and the four best.  A tile without an allowed column: d_cand_val -inf, d_cand_idx 0x7fffffff, d_cand_sum exactly 0, list
 * entries (-inf, 0x7fffffff).  Runs the ids (d_cand_sum NULL), scored or alternatives form by which outputs are non-null.
 * N a multiple of 128.  d_tok_mask = d_set_of_row = NULL is mocr_op_gemm_topk. */
int mocr_op_gemm_argmax_masked(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                               int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                               int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                               const int32_t* d_rowmap);
/* The LM head with a target column (forced prefixes): mocr_op_gemm_argmax_masked (scored or alternatives form) plus d_prefix
 * int32 [rows][prefix_ld] and d_prefix_len int32 [rows], by ROW, d_step int32 [M] and d_tgt_val float32 [M], by slot.  For
 * GEMM row m with row = d_rowmap[m] and t = d_step[m] < d_prefix_len[row], the target column is d_prefix[row][t] and
 * d_tgt_val[m] = its acc + bias (the fp32 value d_cand_val holds when that column wins its tile), -inf when the row's set
 * leaves it out; other entries of d_tgt_val are not written.  Every other output is bit-identical to
 * mocr_op_gemm_argmax_masked's.  The five new arguments all NULL / 0 is that call. */
int mocr_op_gemm_argmax_target(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                               int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                               int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                               const int32_t* d_rowmap, const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld,
                               const int32_t* d_step, float* d_tgt_val);
/* The LM head with edge weights (soft token automata): mocr_op_gemm_argmax_target plus `soft` - d_aut_state int32 [rows] by ROW
 * (the global state every row is in; < 0: none / dead) and the tables d_edge_begin [states + 1], d_edge_token [edges] (a state's
 * tokens strictly ascending), d_edge_weight float32 [edges].  GEMM row m in state s = d_aut_state[d_rowmap[m]] >= 0 has the
 * weight of every edge of s added to its column before the tile is reduced; needs d_tok_mask.  soft = NULL is that call. */
typedef struct mocr_soft_tables {
    int32_t struct_size;        /* sizeof(mocr_soft_tables) */
    const int32_t* d_aut_state;
    const int32_t* d_edge_begin;
    const int32_t* d_edge_token;
    const float* d_edge_weight;
} mocr_soft_tables;
int mocr_op_gemm_argmax_soft(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                             int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                             int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                             const int32_t* d_rowmap, const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld,
                             const int32_t* d_step, float* d_tgt_val, const mocr_soft_tables* soft);
/* The LM head with a repetition penalty: mocr_op_gemm_argmax_soft plus d_seen_mask uint32 [rows][N / 32] and d_penalty_of_row
 * float32 [rows], both by ROW (read through d_rowmap) and both or neither; needs d_tok_mask.  A column whose bit is set takes
 * v < 0 ? v * p : v / p of v = (acc + edge weight) + bias before the mask applies, in the arg-max, the exp sums, the four best
 * and d_tgt_val.  Both NULL is mocr_op_gemm_argmax_soft; soft = NULL with the two set is a penalty without any automaton. */
int mocr_op_gemm_argmax_penalty(mocr_engine* e, const void* dA, const void* dW, const float* d_bias, float* d_cand_val,
                                int32_t* d_cand_idx, float* d_cand_sum, float* d_top_val, int32_t* d_top_idx, int32_t M, int32_t N,
                                int32_t K, int32_t tile, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                                const int32_t* d_rowmap, const int32_t* d_prefix, const int32_t* d_prefix_len, int32_t prefix_ld,
                                const int32_t* d_step, float* d_tgt_val, const mocr_soft_tables* soft, const uint32_t* d_seen_mask,
                                const float* d_penalty_of_row);
/* bf16 engines: the small-batch projection (rows <= 32; kernels_smallm.h SmallMParams), one of the (pro, epi) pairs the
 * small-batch decode step launches: (0,0) (1,0) (0,1) (1,2) (1,3). */
typedef struct mocr_smallm_args {
    int32_t struct_size;        /* sizeof(mocr_smallm_args) */
    int32_t pro;                /* 0: A = a_bf16 [rows][K]; 1: A = bf16(LayerNorm(a_f32 [rows][768])) */
    int32_t epi;                /* 0: fp32 raw; 1: fp32 + bias + residual; 2: bf16 gelu(+ bias); 3: fp32 gelu(+ bias) */
    int32_t rows;
    int32_t K;
    int32_t N;
    int32_t ldo;
    const void* a_bf16;
    const float* a_f32;
    const float* ln_g;
    const float* ln_b;
    float* stats_out;           /* nullable: [rows][2] (mean, rstd) of a_f32 */
    const void* w;              /* [N][K] bf16 */
    const float* bias;
    const float* resid;         /* [rows][N] */
    const float* resid_stats;   /* nullable: resid are pre-LayerNorm sums with these (mean, rstd) and resid_g / resid_b */
    const float* resid_g;
    const float* resid_b;
    void* out;                  /* [rows][ldo] */
} mocr_smallm_args;
int mocr_op_smallm_gemm(mocr_engine* e, const mocr_smallm_args* a);

/* bf16 engines: the attention block of the latent decode path (flag-free default for batches above 256 rows), launched as
 * the decode step launches it for one layer: q = x Wq^T + bq and Qt = bf16(q) . wkT per head (one fused launch, or two
 * launches: gemm_dec_q, then a head-batched GEMM), Et = softmax(Qt X^T) X over the keys (bf16 or, on an fp8 engine, e4m3
 * keys), ctx = Et_h Wv_h^T + bv_h per head.  Fused or not, the tile shapes and the GEMM ring depth are chosen by regime_rows
 * as the decode step chooses them by its batch's regime; the attention kernel by the engine's flags.
 * Rows read and written (N = n rounded up to 128):
 *   x_in   rows < N are read (whole tiles); rows >= n do not reach outputs of rows < n.
 *   q      rows < n written on the two-launch path, rows < N read back.
 *   qt     heads 0..11 of rows < n written; the fused launch writes whole tiles, rows < N.  Heads 12..15 are neither
 *          written nor read.
 *   et     heads 0..11 of rows < n written, rows < n rounded up to 64 read.  Heads 12..15 are neither written nor read.
 *   ctx    rows < n written.
 *   keys   slot s reads keys + (rowmap ? rowmap[s] : s) * key_stride, rows 0 .. L-1 with L = step[0] + 1 (self) or
 *          fixed_len (cross).  When L is not a whole key tile, the last tile is fetched in whole 1-KiB pieces that can carry
 *          part of key row L, the row behind the context (the cache position a previous batch may have written); it is
 *          multiplied by probability 0, so it must be readable and FINITE (0 x NaN = NaN): bf16 rows without NaN / Inf,
 *          e4m3 bytes other than 0x7F / 0xFF. */
typedef struct mocr_latent_args {
    int32_t struct_size;        /* sizeof(mocr_latent_args) */
    int32_t self;               /* 1: keys = cache positions 0 .. step[0] (context step[0] + 1); 0: fixed_len keys */
    int32_t n;                  /* decode slots */
    int32_t regime_rows;        /* the row count the kernel choices are made by (the batch's regime); 0 = n */
    int32_t fixed_len;
    const void* x_in;           /* [N][768] bf16 layer input */
    const void* wq;             /* [768][768] bf16 */
    const float* bq;            /* [768] */
    const void* wkT;            /* [768 in][768 out] bf16: (Wk^T) / 8 */
    const void* wv;             /* [768][768] bf16 */
    const float* bv;            /* [768] */
    const void* keys;           /* bf16 rows of 768, or e4m3 bytes (x = e4m3 * sx) on an fp8 engine */
    int64_t key_stride;         /* elements (bytes for e4m3) between two slots' first key */
    const int32_t* step;        /* self: [n], all equal (a batch decodes in lockstep) */
    const int32_t* rowmap;      /* nullable: slot s reads key slot rowmap[s] */
    float sx;                   /* fp8 engines: key scale */
    void* q;                    /* [N][768] bf16 scratch */
    void* qt;                   /* [N][16][768] bf16 */
    void* et;                   /* [N][16][768] bf16 */
    void* ctx;                  /* [n][768] bf16 */
} mocr_latent_args;
int mocr_op_latent_block(mocr_engine* e, const mocr_latent_args* a);

/* Decode-step HIP graphs this engine holds (test hook: the count must stay bounded whatever row counts callers submit). */
int mocr_graph_count(mocr_engine* e);
/* Row compactions this engine has performed (r04): between two chunks of decode steps the unfinished rows of a batch are
 * moved to the first decode slots and the following steps run on fewer slots - the counterpart of the reference's
 * one-generate()-per-crop loop, where a short text stops at its own EOS (TF/generation/utils.py:2929-2937 via
 * src/ui/main_window.py:9801).  Test hook / statistic; MOCR_FLAG_NO_COMPACTION keeps it at 0. */
int64_t mocr_compaction_count(mocr_engine* e);
/* Decode slots x greedy steps enqueued since mocr_create (statistic): the row-steps the decode launches were sized for.  The
 * tokens a caller got (sum of out_len - 1) over this number is the useful fraction of the decode work - 1.0 for the
 * reference's one-generate()-per-crop loop; mean / max length for a lock-step batch without compaction. */
int64_t mocr_decode_slot_steps(mocr_engine* e);
/* LayerNorm folding of the bf16 encoder (r03: the 24 LayerNorms between the persistent layer GEMMs applied in those GEMMs'
 * epilogues, the GEMMs reading bf16(x) instead of bf16(LN(x)); TF/models/vit/modeling_vit.py:266-286 is the unfolded form).
 * mocr_commit_weights measures, on eight probe crops, how much more input-rounding noise that costs on THIS checkpoint's
 * residual stream: *noise_ratio = sqrt(sum (x g rstd)^2 / sum LN(x)^2), worst LayerNorm (~1 on a near-normalised stream,
 * ~|mean| / spread on one with a DC offset).  Returns 1 when fat batches fold (ratio <= 1.5, or MOCR_FLAG_FORCE_LN_FOLD), 0
 * when the LayerNorms stay launches (ratio above, fp32 engine, MOCR_FLAG_NO_LN_FOLD). */
int mocr_ln_fold_state(mocr_engine* e, float* noise_ratio);
/* Free / total bytes of HBM on a device (the Python constructor sizes its default max_batch from it). */
int mocr_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes);

/* ---- per-kernel timing (HIP events on the engine's stream) -------------------------------- */
typedef struct mocr_kernel_stat {
    char name[48];
    int64_t launches;
    double total_ms;     /* sum of event-measured durations */
    double flops;        /* algorithmic FLOPs over those launches (2 per MAC) */
    double bytes;        /* algorithmic HBM bytes over those launches */
} mocr_kernel_stat;

int mocr_profile_enable(mocr_engine* e, int32_t on); /* on: record an event pair around every launch */
int mocr_profile_reset(mocr_engine* e);
int mocr_profile_get(mocr_engine* e, mocr_kernel_stat* out, int32_t cap, int32_t* n_out);

/* ---- beam search -------------------------------------------------------------------------- */
/* generate(num_beams = K, length_penalty, early_stopping, no_repeat_ngram_size) of transformers 5.x
 * (GenerationMixin._beam_search, do_sample = False), per crop: every step takes log_softmax over the full row, sets the
 * tokens the beam's own history bans to -inf (no renormalising), adds the beam's running score (they start as
 * [0, -1e9, ...]) and keeps the 2 K best of the K x vocab accumulated scores.  A candidate stops when its token is EOS or
 * completes generate(max_length) tokens; the next running beams are the best K that did not stop; the stopped ones among
 * the first K enter the finished set with score / (tokens generated) ^ length_penalty; the early-stop heuristic and the
 * end condition are the reference's for early_stopping false / true / "never".
 * TIES: equal accumulated scores go to the lower flat index beam * vocab + token; a new finished sequence whose score
 * equals one already in the set goes behind it.  (torch.topk promises no order, so nothing should rely on an exact tie.)
 * Beam k of crop c is decode row c K + k: a request of n crops is n K rows over n encodings (one encoder pass per crop),
 * so n * K <= max_batch.  A beam request may carry one token set per crop and ask for the hypotheses' token scores (the
 * *_beam_tokens calls below) and token positions (the *_beam_positions calls); it carries no prefixes, alternatives or
 * source array. */
#define MOCR_MAX_BEAMS 4
typedef struct mocr_beam_config {
    int32_t num_beams;              /* K: 2 .. MOCR_MAX_BEAMS */
    float length_penalty;
    int32_t early_stopping;         /* 0 false, 1 true, 2 "never" */
    int32_t no_repeat_ngram_size;   /* 0 = off */
} mocr_beam_config;
/* Outputs (host, except the device twin's): out_ids [n][K][max_len] int32, out_len [n][K] int32, out_score [n][K] float32 =
 * the crop's K finished hypotheses, hypothesis 0 the best, with the reference's sequences_scores.  A slot that never
 * received a finished sequence has len 0 and score -1e9; ids behind a hypothesis' length are pad_id.  Bad arguments
 * (K outside 2 .. MOCR_MAX_BEAMS, n * K > max_batch, early_stopping outside 0 .. 2, a negative n-gram size, a null
 * pointer) return MOCR_ERR_ARG before any work. */
int mocr_recognize_images_beam(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam,
                               int32_t* out_ids, int32_t* out_len, float* out_score);
/* (a sliver region's K slots read pad_id / 0 / -1e9) */
int mocr_recognize_regions_beam(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score);
int mocr_recognize_gray_host_beam(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                  const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score);
/* device pointers, asynchronous like mocr_recognize_device */
int mocr_recognize_device_beam(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                               void* d_out_len, void* d_out_score);

/* Beam search with token sets and token scores: the *_beam calls plus
 *   out_logp  [n][K][max_len] float32, laid out like out_ids (a device pointer for the device twin), nullable;
 *   sets      HOST int32 [n], one handle of mocr_token_set_create per crop or region, nullable = all MOCR_TOKEN_SET_ALL.
 * With both null they ARE the *_beam calls.  An unknown handle returns MOCR_ERR_ARG, like everything the *_beam calls refuse.
 * TOKEN SETS: all K beams of a crop decode under its set.  A token outside the set scores -inf at every step, before the
 * beam's running score is added, and combines with the n-gram bans of the beam's own history (both are -inf) - this is
 * generate(prefix_allowed_tokens_fn = lambda b, ids: allowed), the PrefixConstrainedLogitsProcessor, with EOS a member of
 * every set.  The log_softmax is taken over the FULL row and nothing renormalises, unlike the greedy *_constrained calls,
 * whose softmax is taken over the set.  MOCR_TOKEN_SET_ALL for every crop is the unconstrained search, bit for bit.
 * DEAD CANDIDATES: with a small set (or one the bans emptied) fewer than 2 K accumulated scores can be finite.  A -inf
 * candidate never outranks a finite one and never enters the finished set (-inf < the empty slots' -1e9); among -inf
 * candidates the lower flat index goes first; a running beam that is dead keeps score -inf, its tokens are unspecified
 * but lie in [0, vocab).  The next running beams are the best K of (score, -1e9 on the stopped ones) by value.
 * TOKEN SCORES of hypothesis (c, j) of length len: out_logp[c][j][0] = 0 (the start token is given); for 1 <= t < len the
 * processed log-probability of ids[t] at the step that appended it, from the beam the hypothesis descends from at that
 * step (compute_transition_scores(sequences, scores, beam_indices, normalize_logits = False)): the fp32 value
 * (logit - row max) - log S the selection ranked.  EOS is scored, and so is the last token of a hypothesis that ends by
 * length.  Positions t >= len, and every position of an empty slot (len 0) or of a sliver region, read 0.  The running score
 * is lp + running, one fp32 add per step from 0, so the fp32 sum of out_logp[1 .. len - 1] taken in order IS the accumulated
 * score, and out_score = that sum / (len - 1) ^ length_penalty.  Asking for token scores, or passing sets that are all
 * MOCR_TOKEN_SET_ALL, moves no id, length or sequence score. */
int mocr_recognize_images_beam_tokens(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam,
                                      int32_t* out_ids, int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets);
int mocr_recognize_regions_beam_tokens(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                       int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                       float* out_score, float* out_logp, const int32_t* sets);
int mocr_recognize_gray_host_beam_tokens(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                         const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                         float* out_logp, const int32_t* sets);
int mocr_recognize_device_beam_tokens(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                      void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets);

/* Beam search with token positions: the *_beam_tokens calls plus
 *   out_pos   [n][K][max_len][MOCR_POSITION_FIELDS] float32, laid out like out_ids (a device pointer for the device twin),
 *             nullable.
 * With out_pos null they ARE the *_beam_tokens calls.
 * TOKEN POSITIONS of hypothesis (c, j) of length len: for 1 <= t < len the five fields of "token positions" above, computed
 * from a_vec - the last decoder layer's LayerNorm-1 output - of the step that appended ids[t], taken on the beam the
 * hypothesis descends from at that step (transformers' beam_indices), over the keys of crop c's encoder rows.  That is
 * exactly what a teacher-forced greedy row over the hypothesis' own ids gives.  EOS has a position like any other token.
 * Zeros are written for t = 0 and t >= len, for every position of an empty slot (len 0) and of a sliver region.
 * Asking for positions moves no id, length, sequence score or token score, bit for bit, and a beam batch in which nobody
 * asks launches exactly what it launched before.  How: the decode steps record a_vec by row, as the greedy positions do;
 * the selection keeps, beside ids and the finished set, the group-relative index of the beam that ran every step (one
 * byte per token); the deferred pass behind the batch gathers each hypothesis' queries through that trail. */
int mocr_recognize_images_beam_positions(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam,
                                         int32_t* out_ids, int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets,
                                         float* out_pos);
int mocr_recognize_regions_beam_positions(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                          int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                          float* out_score, float* out_logp, const int32_t* sets, float* out_pos);
int mocr_recognize_gray_host_beam_positions(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                            const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                            float* out_logp, const int32_t* sets, float* out_pos);
int mocr_recognize_device_beam_positions(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                         void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets, void* d_out_pos);

/* ---- beam search under a token automaton ------------------------------------------------------------------------------
 * The K best entries of a lexicon: a beam search whose every beam walks a token automaton - transformers'
 * generate(num_beams = K, prefix_allowed_tokens_fn = f) with f depending on the beam's history; the *_beam_tokens section is
 * its history-free case.
 *   Every crop may bring an automaton: a handle of mocr_automaton_create, or MOCR_AUTOMATON_NONE.  All K beams of the crop
 *     walk that automaton, each with a state of its own; every beam starts in the start state.
 *   THE MASK at the step that chooses token L of beam k, in state s_k: log_softmax over the full row first; a token is -inf
 *     unless it is in A(s_k) AND the crop's token set - A(s) the edge tokens of s plus EOS iff s accepts, A(MOCR_STATE_DEAD)
 *     empty, EOS a member of every token set as in the *_beam_tokens section; the beam's own n-gram bans are -inf as well.
 *     Nothing renormalises: PrefixConstrainedLogitsProcessor word for word, the rule of the *_beam_tokens section with the set
 *     depending on the state.  There is NO dead-end rule here, unlike greedy: a beam whose effective set is empty is a dead
 *     beam, all its candidates are -inf, and the DEAD CANDIDATES rule of the token form handles it - a dead candidate never
 *     enters the finished set, -inf ties go to the lower flat index, the next beams are the best K of (score, -1e9 on the
 *     stopped ones) by value.
 *   THE STATE after the selection: a new running beam made from candidate (parent p, token x) is in next(s_p, x), or in
 *     MOCR_STATE_DEAD where s_p has no such edge (a -inf candidate, or a stopped one carried on at -1e9: EOS is never an
 *     edge).  A hypothesis that enters the finished set keeps s_p if it stopped on EOS (EOS moves nothing) and next(s_p, x)
 *     if it stopped by completing generate(max_length) tokens (the last token walks, as in greedy).  The state moves with the
 *     hypothesis wherever its ids move, the shift under an inserted hypothesis included.  The K old states are read before
 *     any state is written.
 *   Everything else - stopping, the finished set, length_penalty, early_stopping, the heuristic, the ties, the token scores
 *     (the very fp32 value that was ranked), the trail and the positions - is the token form's definition.
 *   Bit-identities, in ids, lengths, sequence scores, token scores and positions: a crop with MOCR_AUTOMATON_NONE inside a batch
 *     that has automaton crops gives the result of the same crop in a token-form batch of the same size; a crop under the
 *     universal automaton gives the same as a crop with MOCR_AUTOMATON_NONE; a one-state automaton whose self-loops are the
 *     members of a token set gives the same as that set passed through `sets`.  A batch in which nobody brings an automaton
 *     launches exactly what it launched before.
 *   out_state int32 [n][K]: for hypothesis (c, j) the state after the hypothesis' last non-EOS token, in the automaton's own
 *     numbering; MOCR_STATE_NONE for a crop without an automaton, for an empty slot (length 0) and for a sliver region.  A
 *     finished hypothesis is never MOCR_STATE_DEAD: its score is finite, so every one of its tokens had an edge.
 *   With fewer reachable entries than K, the slots beyond them hold what the search leaves there: continuations of the
 *     padding beams that start at -1e9 (duplicates that score about -1e9), or nothing.  The calls deliver that as it is.
 *   How: the selection kernel's automaton form (profile names beam_select_am / beam_select_am_tr) builds every beam's mask in
 *     LDS from the edges of its state; one lane per winner finds the next state by binary search.  The tables reach it as one
 *     trailing argument.  The beams' states are the greedy calls' row states; the hypotheses' states (4 B a row and lane) are
 *     allocated by the first beam batch that brings an automaton, and mocr_automaton_state_bytes counts them.
 * The *_beam_automaton entry points: the *_beam_positions twins plus `automata`, a HOST int32 array [n] of handles, one per
 * crop (null: every crop MOCR_AUTOMATON_NONE; copied before the call returns), and out_state int32 [n][K] (nullable; host, or
 * device for the device twin).  With both null they ARE the *_beam_positions calls.  An unknown handle is MOCR_ERR_ARG before
 * any work. */
int mocr_recognize_images_beam_automaton(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam, int32_t* out_ids,
                                         int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                         const int32_t* automata, int32_t* out_state);
int mocr_recognize_regions_beam_automaton(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                          int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                          float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                          const int32_t* automata, int32_t* out_state);
int mocr_recognize_gray_host_beam_automaton(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                            const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                            float* out_logp, const int32_t* sets, float* out_pos, const int32_t* automata,
                                            int32_t* out_state);
int mocr_recognize_device_beam_automaton(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                         void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets, void* d_out_pos,
                                         const int32_t* automata, void* d_out_state);

/* ---- beam search under soft token automata ---------------------------------------------------------------------------
 * transformers' generate(num_beams = K, sequence_bias = ...): the bias is a logits processor applied BEHIND the log_softmax,
 * so it enters the beam's accumulated score and sequences_scores - a glossary re-ranks whole hypotheses instead of one token
 * at a time.  It is the rule of the section above with the automaton allowed to be SOFT (edge_weight / default_next of
 * mocr_automaton_desc), and NOT the greedy soft rule, which adds the weight before its softmax.
 *   THE MASK at the step that chooses token L of beam k, in state s_k:
 *     1. lp = log_softmax over the FULL row of the raw logits: the row's max and log-sum never see a weight;
 *     2. s = lp + edge_weight(s_k, t) in fp32 where s_k has an edge on t, s = lp elsewhere (a zero weight adds nothing);
 *     3. -inf outside A(s_k) AND the crop's token set, and on the beam's n-gram bans;
 *     4. acc = s + the beam's running score.
 *     A(s) of an OPEN state (default_next[s] >= 0) is every non-EOS token, plus EOS iff s accepts; A(s) of a closed state is
 *     the section above's.  Nothing renormalises, a weight never revives a masked token, and there is no dead-end rule.
 *   THE STATE: a candidate (parent p, token x) goes to next(s_p, x) where s_p has an edge on x; else along default_next[s_p] -
 *     with MOCR_DEFAULT_FALLBACK the token is looked up in the default state's edges, one level, exactly as the greedy soft
 *     walk does -; else, only where default_next[s_p] is -1, to MOCR_STATE_DEAD.  A candidate that stopped on EOS and is
 *     carried on at score - 1e9 follows the default edge of an open state like any token without an edge (EOS is never an
 *     edge, so under the fallback form it lands on the default state - transformers' suffix match restarts), and is
 *     MOCR_STATE_DEAD in a closed state.  The hypotheses' states move as in the section above.
 *   TOKEN SCORES are the very fp32 value that was ranked, s = lp + w (compute_transition_scores(normalize_logits = False)):
 *     running' = s + running holds exactly, and the sequential fp32 sum of a hypothesis' token scores over
 *     (len - 1) ^ length_penalty IS its score.
 *   Bit-identities, in ids, lengths, sequence scores, token scores, positions and states: a hard automaton created with
 *     all-zero weights equals the same automaton created without, inside a soft beam batch; the universal-open automaton (one
 *     accepting open state, default_next = 0, no edges) equals MOCR_AUTOMATON_NONE; hard and plain crops of a soft beam batch
 *     equal the same crops in a *_beam_automaton batch of the same size; a beam batch in which no crop brings a soft automaton
 *     launches exactly what it launched before.
 *   How: the selection kernel's SOFT form (profile names beam_select_sw / beam_select_sw_tr), chosen iff a crop of the batch
 *     brings a soft handle.  A thread binary-searches the state's ascending edge tokens once per float4 of the row it holds
 *     and adds the weights inside it; the winners' lanes take the weight of the edge they find.  The arena's two soft arrays
 *     reach it in the trailing argument; no buffer is new, and mocr_automaton_state_bytes does not move.
 *   Out of scope: weights on EOS, non-finite weights, two automata per crop, more than MOCR_MAX_BEAMS beams.
 * The *_beam_soft entry points: the argument lists of the *_beam_automaton twins; `automata` may hold soft handles.  With no
 * soft handle among them a *_beam_soft call IS the *_beam_automaton call: the same launches, the same bits. */
int mocr_recognize_images_beam_soft(mocr_engine* e, const mocr_image* images, int32_t n, const mocr_beam_config* beam, int32_t* out_ids,
                                    int32_t* out_len, float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                    const int32_t* automata, int32_t* out_state);
int mocr_recognize_regions_beam_soft(mocr_engine* e, const mocr_image* pages, int32_t n_pages, const mocr_region* regions,
                                     int32_t n_regions, const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len,
                                     float* out_score, float* out_logp, const int32_t* sets, float* out_pos,
                                     const int32_t* automata, int32_t* out_state);
int mocr_recognize_gray_host_beam_soft(mocr_engine* e, const uint8_t* gray, int32_t n, int32_t max_len_override,
                                       const mocr_beam_config* beam, int32_t* out_ids, int32_t* out_len, float* out_score,
                                       float* out_logp, const int32_t* sets, float* out_pos, const int32_t* automata,
                                       int32_t* out_state);
int mocr_recognize_device_beam_soft(mocr_engine* e, const void* d_gray, int32_t n, const mocr_beam_config* beam, void* d_out_ids,
                                    void* d_out_len, void* d_out_score, void* d_out_logp, const int32_t* sets, void* d_out_pos,
                                    const int32_t* automata, void* d_out_state);

/* Bytes of beam state this engine holds, over its lanes (test hook): 0 until a lane runs its first beam batch - creating an
 * engine and greedy calls of any kind allocate none of it. */
int64_t mocr_beam_state_bytes(mocr_engine* e);
/* ... and of the token form's two histories, which mocr_beam_state_bytes does not count: 0 until a lane runs its first beam
 * batch that asks for token scores or brings a set other than MOCR_TOKEN_SET_ALL. */
int64_t mocr_beam_token_state_bytes(mocr_engine* e);
/* ... and of the two beam-index trails, which neither of the two counts: 0 until a lane runs its first beam batch that asks
 * for token positions.  (The buffers of the token positions themselves are those of the greedy *_positions calls.) */
int64_t mocr_beam_position_state_bytes(mocr_engine* e);
/* The first n entries of a lane's decode slot -> row map as its last batch left it (test hook; all lanes idle first): behind
 * a compacted beam batch the K rows of a crop still sit in K neighbouring slots, in beam order, from a slot that is a
 * multiple of K. */
int mocr_lane_rowmap(mocr_engine* e, int32_t lane, int32_t* out_rowmap, int32_t n);

/* The selection that ends a beam step (kernel unit tests): the token-step arguments on the slab path (no first, forced or
 * candidate form; a->n slots = groups of K, a trailing partial group is padding), plus the beam state by ROW like ids:
 * d_beam_score / d_parent / d_hyp_len / d_hyp_score [rows], d_hyp_ids [rows][ids_ld], d_heuristic_open [rows / K]. */
int mocr_op_beam_select(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score,
                        int32_t* d_parent, int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open);
/* ... in its token form: plus d_beam_logp / d_hyp_logp [rows][ids_ld] float32 (both or neither) and d_tok_mask
 * [sets][vocab / 32] with d_set_of_row [rows] (both or neither; every entry a row of d_tok_mask, the K rows of a crop naming one set).  With all four null it is
 * mocr_op_beam_select. */
int mocr_op_beam_select_tokens(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score,
                               int32_t* d_parent, int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open,
                               float* d_beam_logp, float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row);
/* ... in its trail form: plus d_beam_trail / d_hyp_trail, uint8 [rows][ids_ld] (both or neither).  d_beam_trail[row][t],
 * t >= 1, is the beam 0 .. K - 1 of the crop's group whose row ran the step that appended ids[row][t]; it moves with ids,
 * and the entry of the token a step appends is the candidate's parent.  d_hyp_trail moves with d_hyp_ids, 0 behind a
 * hypothesis' length.  With both null it is mocr_op_beam_select_tokens. */
int mocr_op_beam_select_positions(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score,
                                  int32_t* d_parent, int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open,
                                  float* d_beam_logp, float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                                  uint8_t* d_beam_trail, uint8_t* d_hyp_trail);
/* ... under token automata: mocr_op_beam_select_positions plus the CSR tables over global state numbers (as
 * mocr_op_dec_token_automaton takes them), d_aut_base_of_row [rows] (the crop's start state, -1: none), d_aut_state [rows] (in /
 * out: the running beams' states) and d_hyp_state [rows] (in / out: the finished hypotheses' states, by crop K + slot).  All
 * seven null: it IS mocr_op_beam_select_positions; otherwise all seven set. */
int mocr_op_beam_select_automaton(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score,
                                  int32_t* d_parent, int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open,
                                  float* d_beam_logp, float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row,
                                  uint8_t* d_beam_trail, uint8_t* d_hyp_trail, const int32_t* d_edge_begin, const int32_t* d_edge_token,
                                  const int32_t* d_edge_next, const uint8_t* d_accepting, const int32_t* d_aut_base_of_row,
                                  int32_t* d_aut_state, int32_t* d_hyp_state);
/* ... under soft token automata: mocr_op_beam_select_automaton plus d_edge_weight float32 [edges] and d_default_next int32
 * [states] over global state numbers (MOCR_DEFAULT_FALLBACK as in the arena; -1: closed), both or neither, and only with the
 * seven automaton pointers.  Both null: it IS mocr_op_beam_select_automaton. */
int mocr_op_beam_select_soft(mocr_engine* e, const mocr_token_args* a, const mocr_beam_config* beam, float* d_beam_score, int32_t* d_parent,
                             int32_t* d_hyp_ids, int32_t* d_hyp_len, float* d_hyp_score, int32_t* d_heuristic_open, float* d_beam_logp,
                             float* d_hyp_logp, const uint32_t* d_tok_mask, const int32_t* d_set_of_row, uint8_t* d_beam_trail,
                             uint8_t* d_hyp_trail, const int32_t* d_edge_begin, const int32_t* d_edge_token, const int32_t* d_edge_next,
                             const uint8_t* d_accepting, const int32_t* d_aut_base_of_row, int32_t* d_aut_state, int32_t* d_hyp_state,
                             const float* d_edge_weight, const int32_t* d_default_next);
/* The cache reorder behind it: d_cache viewed as [layers][rows][segs][positions][pos_bytes] through byte strides; for
 * every group of K slots whose crop is live (d_finished[rowmap[g K]] == 0), row rowmap[g K + k] <- row
 * rowmap[g K + d_parent[rowmap[g K + k]]], bytes 0 .. d_step[g K] * pos_bytes - 1 of every (layer, segment).  max_pos bounds
 * every step (the grid). */
int mocr_op_beam_permute(mocr_engine* e, void* d_cache, int32_t layers, int64_t layer_stride, int64_t row_stride, int32_t segs,
                         int64_t seg_stride, int32_t pos_bytes, int32_t K, const int32_t* d_parent, const int32_t* d_rowmap,
                         const int32_t* d_finished, const int32_t* d_step, int32_t n_slots, int32_t max_pos);

#ifdef __cplusplus
}
#endif
#endif /* MOCR_H */
