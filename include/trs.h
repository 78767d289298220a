/*
 * trs.h — C-ABI of libtrs_hip.so: the MI355X (gfx950) hot path of the torchrecsys training loop.
 *
 * The reference (FrancescoI/torchrecsys) has no FFI; the seams this library sits behind are Python call
 * contracts.  Every entry point below names the reference interface it replaces
 * (file:line relative to the reference tree).  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add to bind them.
 *
 * Conventions
 *  - every pointer named *_dev / inside trs_tables / trs_batch is a DEVICE pointer owned by the caller
 *    (PyTorch-ROCm allocates; the library never allocates, frees or synchronises);
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null stream) and is
 *    safe to capture into a hipGraph;
 *  - return value: 0 = OK, negative = TRS_E_* ; trs_last_error() gives the message of the calling thread's
 *    last failure.  No C++ exception crosses the boundary;
 *  - ids are int32 or int64 (`idx_bytes` = 4 or 8): the reference uses int64 everywhere
 *    (dataset/dataset.py:268-269), the device-resident interaction stream uses int32;
 *  - an id outside its table is never dereferenced: the triple is skipped and bit 0 of *err_flag_dev is set
 *    (the reference raises IndexError from aten::embedding; the host mirror raises it at the next sync);
 *  - "field" order of every per-triple staging array: 0 = user, 1 = pos item, 2 = neg item,
 *    3+2m = pos metadata column m, 4+2m = neg metadata column m  (R = 3 + 2M fields).
 */
#ifndef TRS_H
#define TRS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_MAX_META 8
#define TRS_MAX_LAYERS 8

#define TRS_OK 0
#define TRS_E_ARG (-1)     /* bad argument (shape, NULL, unsupported size) */
#define TRS_E_LAUNCH (-2)  /* HIP launch / runtime error */
#define TRS_E_DEVICE (-3)  /* no gfx950 device / wrong architecture */

#define TRS_NET_LINEAR 0
#define TRS_NET_FM 1

/* Pairwise training loss over (positive score, negative score), mean over the batch.  HINGE is the reference's
 * (helper/loss.py:5-9: clamp(neg - pos + 1, min=0)); BPR = -log sigmoid(pos - neg) is the alternative BASELINE.json's
 * north_star names — the reference has no such loss and fit() no loss argument, so BPR is pinned by its formula
 * (oracle/nets.py::bpr_loss against torch autograd), not by reference outputs. */
#define TRS_LOSS_HINGE 0
#define TRS_LOSS_BPR 1
/* Sampled softmax over one positive and K sampled negatives per row (trs_score_multi_fwd_bwd only; not a pair loss). */
#define TRS_LOSS_SAMPLED_SOFTMAX 2
/* WARP, the rank-weighted first violator among K sampled negatives (trs_score_warp_fwd_bwd only; not a pair loss). */
#define TRS_LOSS_WARP 3

/* Embedding tables of one scorer.  Row-major (n_rows, D) fp32, as nn.Embedding.weight
 * (embeddings/init_embeddings.py:5-50,53-97).
 *   Linear (collaborative/linear.py:43-51): user,item = self.user,self.item; user_lin,item_lin = user_bias,item_bias
 *                                           (n,1); meta[m] = self.metadata[m]; meta_lin unused (NULL).
 *   FM     (collaborative/fm.py:42-56):     user,item; user_lin,item_lin = linear_user,linear_item (n,1);
 *                                           meta[m] = metadata[m]; meta_lin[m] = linear_metadata[m] (n,1).
 *   MLP    (collaborative/mlp.py:66-71):    user,item; meta[m] = metadata_embeddings[m]; *_lin unused. */
typedef struct trs_tables {
  float* user;
  float* item;
  float* user_lin;
  float* item_lin;
  float* meta[TRS_MAX_META];
  float* meta_lin[TRS_MAX_META];
  int64_t n_users;
  int64_t n_items;
  int64_t n_meta[TRS_MAX_META];
  int32_t D; /* n_factors */
  int32_t M; /* metadata columns, 0..TRS_MAX_META */
} trs_tables;

/* One mini-batch as FastDataLoader.__next__ yields it (dataset/dataset.py:414-458):
 * keys user_id, pos_item_id, neg_item_id (B,), pos_metadata_id, neg_metadata_id (B,M) row-major. */
typedef struct trs_batch {
  const void* user;
  const void* pos;
  const void* neg;      /* NULL: score the positive pass only (predict, model.py:436-439) */
  const void* pos_meta; /* (B,M) or NULL when M == 0 */
  const void* neg_meta;
  int64_t B;
  int32_t idx_bytes;     /* 4 or 8 */
  int32_t* err_flag_dev; /* optional; bit 0 set on an out-of-range id */
} trs_batch;

/* ---------------------------------------------------------------------------------------------- misc */
const char* trs_last_error(void);
/* ABI version of this header; bump on ANY signature or struct-layout change.  The ctypes binding refuses a library
 * whose trs_abi_version() differs (torchrecsys_amd/_lib.py::load), tests/test_abi.py checks the three copies agree.
 *   1: round 1.   2: trs_train_steps_sgd takes a trs_train_args struct; trs_epoch_presort writes item-duplicate flags.
 *   3: trs_bn_relu_forward (running statistics, batch counter, output-layer dot) and trs_bn_relu_backward (outer-product
 *      form, outer_xw) grew arguments; trs_hinge_auc_backward, trs_f32_to_bf16_multi, trs_mlp_embed_sgd_update added.
 *   4: trs_sampler.seen_users (bounds of the seen CSR); trs_train_args.sync_dev (flag mode as one launch per step);
 *      trs_mlp_gather_gemm1_fwd, trs_tuning_set added; trs_epoch_flags takes batches up to 262 144; the presort entry
 *      points no longer use their temp buffers (no vendor sort).
 *   5: trs_epoch_flags_ordered (flagged-first batches), trs_train_args.n_flagged_dev.
 *   6: batched top-k retrieval: trs_csr, trs_item_fold(_bytes), trs_retrieve_topk, trs_retrieve_workspace_bytes,
 *      trs_mask_seen, trs_rank_metrics.  (Entry points added since without touching an existing signature or struct:
 *      the in-batch softmax group, trs_batch_prepare_mined, trs_batch_prepare_multi, trs_score_multi_fwd_bwd,
 *      trs_score_warp_fwd_bwd, TRS_LOSS_WARP, trs_stage_add_l2, trs_neighbour_fold, trs_neighbours_topk,
 *      trs_fold_in_users, trs_item_ranks, trs_item_ranks_workspace_bytes, trs_mmr_rerank, trs_list_ild,
 *      trs_fold_in_items, trs_als_gram, trs_als_gram_workspace_bytes, trs_als_solve, trs_ease_gram, trs_ease_invert,
 *      trs_ease_invert_workspace_bytes, trs_ease_weights, trs_ease_scores, trs_seq_fwd_bwd, trs_seq_user_rows,
 *      trs_lgcn_propagate, trs_lgcn_adam, trs_knn_build, trs_knn_build_workspace_bytes, trs_knn_scores.) */
#define TRS_ABI_VERSION 6
#define TRS_SYNC_WORDS 288
#define TRS_SYNC_REBASE 0x40000000u /* arrivals after which trs_train_steps_sgd zeroes sync_dev and its host count */
int trs_abi_version(void);
/* Tuning / A-B knobs of the launch paths (kernel selection, launch shapes): GRID_CAP, PASS_GRID_CAP, K1_ITERS,
 * PASS_ITERS, PRESORT_GRID_CAP, PASS_NT, K1_NT, K1_WGS_PER_CU, K1_APPLY_IN_LOOP, K1_APPLY_STATS, GEMM32_NO_GLDS,
 * GEMM16_TN_WIDE, GEMM16_TILE, GEMM16_NO_GLDS, BN_FINAL_TWO_SWEEPS, FOLDIN_DEPTH, RANKS_STAGES, EASE_STAGES (meanings:
 * csrc/trs_common.h TrsTuning).  The library reads TRS_<name> from the environment ONCE, at its first use; this entry
 * point changes a knob afterwards (tests, tools): unset != 0 restores the default.  The defaults are the measured best. */
int trs_tuning_set(const char* name, int64_t value, int32_t unset);
/* 0 if the current HIP device is gfx950, TRS_E_DEVICE otherwise. */
int trs_check_device(void);

/* HIP timing events owned by the library (bench.py times the dominant kernel with them on the launch stream).
 * create: n new events; elapsed_ms: host-side read after the stream was synchronised. */
int trs_events_create(int32_t n, void** handles_out);
int trs_events_destroy(int32_t n, void** handles);
int trs_events_elapsed_ms(void* start, void* stop, float* ms_out);

/* ------------------------------------------------------------------------- loader / sampler (a9, a10) */
/* Sampler options beyond the reference's (the reference only rejects the row's own positive,
 * dataset/dataset.py:435-447).  NULL everywhere below = the reference's sampler.  Counter-based like the plain sampler
 * (try 0 with every option off IS the plain sampler's draw):
 *   k_neg      every interaction is visited k_neg times per epoch, each time with a fresh negative: the epoch has
 *              N * k_neg positions, position q maps to row perm_{N*k_neg}(q) % N;
 *   popularity candidates are drawn as the item of a uniformly random interaction (pop_items[r], r < pop_n), i.e.
 *              proportionally to the item's frequency in the stream, instead of uniformly over the catalogue;
 *   seen_off / seen_items   CSR of every user's positives (seen_off (n_users+1), seen_items sorted per user): a
 *              candidate the user has interacted with is rejected and redrawn (key = seed + try * golden ratio), at
 *              most max_tries candidates; the last one is kept whatever it is (bounded work).
 * The negative always differs from the row's positive. */
typedef struct trs_sampler {
  int32_t k_neg;      /* >= 1 */
  int32_t popularity; /* 0 | 1 */
  int32_t max_tries;  /* >= 1 */
  int32_t reserved;
  const int64_t* seen_off;
  const int32_t* seen_items;
  const int32_t* pop_items;
  int64_t pop_n;
  int64_t seen_users; /* rows of the seen CSR = n_users; a user id outside [0, seen_users) has seen nothing */
} trs_sampler;

/* Counter-based dynamic negative sampler: neg[t] uniform over {0..n_items-1} \ {pos[t]} — the distribution of the
 * rejection loop at dataset/dataset.py:440-445 (reject only the row's own positive).  Stream: Philox4x32-10,
 * key = seed, counter = offset + t; r = mulhi64(x, n_items-1); neg = r + (r >= pos).  Not the numpy legacy
 * stream (that one is replayed on the host by FastDataLoader for bit-exact reference batches). */
int trs_sample_neg(const void* pos_dev, int idx_bytes, int64_t B, int64_t n_items, uint64_t seed,
                   uint64_t offset, void* neg_out_dev, void* stream);

/* Epoch shuffle + batch slice + negative sampling in one pass over a device-resident interaction stream
 * (replaces torch.randperm + tensor[perm[i:i+B]] at dataset/dataset.py:364-373,420-422 and the sampler loop
 * :435-447).  Row p of the stream is (stream_user[p], stream_item[p]), int32.  Position q = t0 + t of the epoch maps
 * to row perm(q) where perm is a keyed bijection of [0,N) (4-round Feistel network over ceil(log2 N) bits with
 * cycle walking, round function Philox-mix keyed by shuffle_key; shuffle_key = 0 means identity = shuffle=False).
 * Writes user/pos/neg int32 (B,) and, when M > 0, pos_meta/neg_meta (B,M) looked up through item_meta (n_items,M)
 * (the device form of item_to_metadata_map, dataset/dataset.py:375-411).  neg_static (N,) int32 non-NULL selects the
 * static negatives of dataset/dataset.py:56-64 instead of sampling. */
int trs_batch_prepare(const int32_t* stream_user_dev, const int32_t* stream_item_dev,
                      const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key, int64_t t0, int64_t B,
                      int64_t n_items, uint64_t sample_seed, uint64_t sample_offset,
                      const int32_t* item_meta_dev, int32_t M, int32_t* user_out, int32_t* pos_out,
                      int32_t* neg_out, int32_t* pos_meta_out, int32_t* neg_meta_out, const trs_sampler* sampler,
                      void* stream);

/* trs_batch_prepare with score-aware hard-negative mining (dynamic negative sampling, Zhang et al., SIGIR 2013; the
 * reference has no such sampler): per triple, `candidates` = K negatives are drawn, scored under the tables AS THEY ARE
 * when the launch runs, and one of the `top` = m highest-scoring ones becomes the triple's negative.  One launch.
 * For epoch position q (user u, positive p as trs_batch_prepare derives them), sampler seed s = sample_seed and
 * ctr = sample_offset + t, the Philox counter trs_batch_prepare uses for that position:
 *   candidates  c_j = the sampler's draw (popularity / seen rejection / max_tries of `sampler` unchanged; every c_j
 *               differs from p) under the seed s_j = (s + j * 0xD1B54A32D192ED03) mod 2^64, j = 0 .. K-1; the retry keys
 *               inside a draw are s_j + t * 0x9E3779B97F4A7C15, and all (j, t) offsets for j <= 65, t <= 64 are distinct
 *               mod 2^64.  c_0 is exactly the negative trs_batch_prepare writes.  Candidates may repeat.
 *   scores      z_j = the scorer's negative-pass value of (u, c_j, metadata of c_j through item_meta): net =
 *               TRS_NET_LINEAR the score, TRS_NET_FM the value BEFORE the sigmoid (strict where fp32 sigmoid saturates,
 *               as retrieval ranks) — the arithmetic of trs_score_forward, bit for bit.
 *   choice      candidates ordered by (z_j descending, j ascending; NaN first as torch.sort, -0.0 = +0.0); the negative
 *               is the candidate of rank r, r = 0 if m == 1, else r = mulhi64(x, m) with x = words (y << 32 | x) of
 *               Philox(ctr, s_K) (uniform over the m best: the usual guard against false negatives).
 * Outputs as trs_batch_prepare (user, pos, the mined neg, both metadata rows when M > 0) and, when chosen_out (B) int32
 * is given, the chosen candidate's index j.  candidates == 1 reproduces trs_batch_prepare bit for bit.  k_neg composes
 * unchanged (positions, counters and the shuffle are those of the unmined epoch).  An id of the stream outside its
 * table is never used as a row index here (the scorer of the step reports it).
 * TRS_E_ARG, nothing launched: tables NULL; net not TRS_NET_LINEAR / TRS_NET_FM; candidates outside 1..64; top outside
 * 1..candidates; neg_static given; M != tables->M, or M > 0 without item_meta or the metadata outputs; a D the scorer
 * kernels do not take; NULL tables' members; n_items > tables->n_items. */
int trs_batch_prepare_mined(const int32_t* stream_user_dev, const int32_t* stream_item_dev,
                            const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key, int64_t t0, int64_t B,
                            int64_t n_items, uint64_t sample_seed, uint64_t sample_offset,
                            const int32_t* item_meta_dev, int32_t M, int32_t* user_out, int32_t* pos_out,
                            int32_t* neg_out, int32_t* pos_meta_out, int32_t* neg_meta_out, const trs_sampler* sampler,
                            int net, const trs_tables* tables, int32_t candidates, int32_t top, int32_t* chosen_out,
                            void* stream);

/* trs_batch_prepare for K = n_neg sampled negatives per positive.  One launch: epoch shuffle ->
 * (user u, positive p) -> K draws; no table row is read.  For epoch position q = t0 + t, seed s = sample_seed and
 * ctr = sample_offset + t (the Philox counter trs_batch_prepare uses for that position), candidate
 *   c_j = the sampler's draw (popularity / seen rejection / max_tries / k_neg of `sampler` unchanged; c_j != p) under the
 *         seed s_j = (s + j * 0xD1B54A32D192ED03) mod 2^64, j = 0 .. K-1 — the candidate schedule of
 *         trs_batch_prepare_mined; c_0 is exactly the negative trs_batch_prepare writes.  Candidates may repeat inside a
 *         row (sampling with replacement).
 * Outputs, all int32: user_out (B); items_out (1+K, B) slot-major — row 0 the positives, row 1+j candidate j — so the
 * COO index list of the item tables is the block itself; meta_out (1+K, B, M) when M > 0: the metadata ids of the item
 * in the same slot, looked up through item_meta (n_items, M).  With n_neg = 1, items_out = [pos; neg] and meta_out =
 * [pos_meta; neg_meta] of trs_batch_prepare, bit for bit.  An id of the stream outside [0, n_items) is never used as an
 * index here (the scorer reports it).
 * TRS_E_ARG, nothing launched: n_neg outside 1..64; neg_static given (no static negatives); M outside
 * 0..TRS_MAX_META, or M > 0 without item_meta / meta_out; the slice outside the epoch; bad sampler options; n_items < 2;
 * NULL streams or outputs with B > 0. */
int trs_batch_prepare_multi(const int32_t* stream_user_dev, const int32_t* stream_item_dev,
                            const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key, int64_t t0, int64_t B,
                            int64_t n_items, uint64_t sample_seed, uint64_t sample_offset,
                            const int32_t* item_meta_dev, int32_t M, int32_t* user_out, int32_t* items_out,
                            int32_t* meta_out, const trs_sampler* sampler, int32_t n_neg, void* stream);

/* One training pass of a Linear / FM scorer over rows of one positive and K sampled negatives (the id blocks of
 * trs_batch_prepare_multi: user (B), items (1+K, B), meta (1+K, B, M), int32), all rows read from the PRE-update tables.
 * z(u, i) is the scorer's value of (u, i, metadata of i): Linear the score, FM the argument of its sigmoid — the
 * arithmetic of trs_score_forward, bit for bit (FM scores below are sigmoid(z)).
 *   loss = TRS_LOSS_SAMPLED_SOFTMAX: zh_0 = z(u,p)/tau, zh_{1+j} = z(u,c_j)/tau; row loss = logsumexp_s zh_s - zh_0;
 *     d loss / d zh_s = (softmax_s - [s == 0]) * inv_B (row maximum subtracted); every occurrence of a repeated
 *     candidate counts.  The user's 1-wide gradient is written as exactly 0 (z's derivative by it is 1 in every slot).
 *   loss = TRS_LOSS_HINGE / TRS_LOSS_BPR: row loss = (1/K) sum_j pair(score_p, score_cj) of trs_score_fwd_bwd's pair
 *     loss; tau is ignored.  With K = 1 the staged gradients and the loss are those of trs_score_fwd_bwd, bit for bit.
 * loss_sum += the sum of the row losses (the caller divides by B); auc_count (may be NULL) += #(score_p > score_c0).
 * Both are ACCUMULATED.  inv_B = 1/B of the mean.
 * Staged gradients, field-major, F = 1 + (1+K)(1+M) fields: grad_rows (F, B, D) and grad_lin (F, B); field 0 the user,
 * field 1+s the item of slot s, field 1+(1+K)+m*(1+K)+s the metadata column m of slot s — every table's entries are one
 * contiguous ((1+K)*B, D) block in the order of its id block.  Linear has no 1-wide metadata tables: those fields are 0.
 * grad_rows == NULL (then grad_lin must be NULL too): forward only — the same loss and AUC count, nothing staged.
 * An id outside its table is clamped for addressing, sets bit 0 of *err_flag_dev (may be NULL) and zeroes its row's
 * loss and gradients.
 * TRS_E_ARG, nothing launched: tables NULL or a NULL member; net not TRS_NET_LINEAR / TRS_NET_FM; K outside 1..64; an
 * unknown loss id; M != tables->M; a D the scorer kernels do not take; tau <= 0 or not finite; loss_sum NULL; grad_lin
 * without grad_rows or the reverse; NULL ids with B > 0. */
int trs_score_multi_fwd_bwd(int net, const trs_tables* tables, const int32_t* user_dev, const int32_t* items_dev,
                            const int32_t* meta_dev, int64_t B, int32_t M, int32_t K, int32_t loss, float tau,
                            float inv_B, float* loss_sum_dev, int32_t* auc_count_dev, float* grad_rows_dev,
                            float* grad_lin_dev, int32_t* err_flag_dev, void* stream);

/* WARP (Weighted Approximate-Rank Pairwise loss, Weston et al. 2011: WSABIE) of a Linear / FM scorer over
 * rows of one positive p and K candidates c_0 .. c_{K-1} (the id blocks of trs_batch_prepare_multi, unchanged: user (B),
 * items (1+K, B), meta (1+K, B, M), int32), all rows read from the PRE-update tables.  z(u, i) is pass_forward_z's value:
 * Linear the score, FM the argument of its sigmoid (as sampled softmax, mining and retrieval; on the sigmoid itself a
 * margin of 1 would always be violated).
 *   violation  h_j = (z(u,c_j) - z(u,p)) + margin; candidate j violates iff h_j > 0 (a NaN does not); J = the smallest
 *              violating j; trials = J + 1, or 0 when no candidate violates.
 *   weight     w = rank_weight[J]: K floats on the device, supplied by the caller (the rank estimate of a row that needed
 *              J + 1 draws; no clipping).
 *   loss       row loss = w * h_J, or 0 without a violator.  d loss / d z(u,c_J) = +w * inv_B, d loss / d z(u,p) =
 *              -w * inv_B (no sigmoid factor), through z's derivatives.  The user's 1-wide term enters both z with
 *              derivative 1: its gradient is written as exactly 0.
 * loss_sum += the sum of the row losses (the caller divides by B); auc_count (may be NULL) += #(score_p > score_c0), on
 * the scores trs_score_fwd_bwd counts (FM: sigmoid(z)).  Both are ACCUMULATED.
 * Outputs: neg_out (B) the chosen candidate c_J's id and neg_meta_out (B, M) its metadata ids (c_0's without a violator,
 * so the index lists stay valid); trials_out (B, may be NULL).  Staged gradients in trs_score_fwd_bwd's order, R = 3 + 2M
 * fields: grad_rows (R, B, D) and grad_lin (R, B) — user, positive, chosen candidate, then per metadata column the
 * positive's and the chosen candidate's; the positive's ids are slot 0 of the input blocks.  A row without a violator
 * stages zeros.  Linear has no 1-wide metadata tables: those fields are 0.
 * grad_rows == NULL (then grad_lin must be NULL too): forward only — the same loss, AUC count, neg_out, neg_meta_out and
 * trials_out, nothing staged.
 * An id outside its table is clamped for addressing, sets bit 0 of *err_flag_dev (may be NULL) and zeroes its row's loss
 * and gradients; its trials = 0 and its neg_out = c_0 as given.
 * TRS_E_ARG, nothing launched: the grounds of trs_score_multi_fwd_bwd (tables NULL or a NULL member; net not
 * TRS_NET_LINEAR / TRS_NET_FM; K outside 1..64; M != tables->M; a D the scorer kernels do not take; loss_sum NULL;
 * grad_lin without grad_rows or the reverse; NULL ids with B > 0) and: margin not finite; rank_weight NULL; neg_out NULL
 * (or neg_meta_out NULL with M > 0). */
int trs_score_warp_fwd_bwd(int net, const trs_tables* tables, const int32_t* user_dev, const int32_t* items_dev,
                           const int32_t* meta_dev, int64_t B, int32_t M, int32_t K, float margin,
                           const float* rank_weight_dev, float inv_B, float* loss_sum_dev, int32_t* auc_count_dev,
                           int32_t* neg_out, int32_t* neg_meta_out, int32_t* trials_out, float* grad_rows_dev,
                           float* grad_lin_dev, int32_t* err_flag_dev, void* stream);

/* Per-sample L2 regularisation of the embedding rows a batch references: one pass over the field-major
 * staging buffer of a Linear / FM step, after the staging kernel and before the first row update, so the rows it reads
 * are the PRE-update tables'.  Ids are the blocks of trs_batch_prepare_multi, int32: user (B), items (S, B), meta
 * (S, B, M).  Fields, F = 1 + S(1+M): grad_rows (F, B, D) and grad_lin (F, B); field 0 the user, field 1+s the item of
 * slot s, field 1+S+m*S+s metadata column m of slot s — S = 1 is the in-batch softmax's buffer, S = 2 a pair's or the
 * WARP triple's (trs_score_fwd_bwd's order), S = 1+K trs_score_multi_fwd_bwd's.  For every reference (f, t) with id r
 * in the table of its group (user / item / metadata):
 *   grad_rows[f, t, :] = grad_rows[f, t, :] + c_group * W[r, :]     (the product, then the sum: two fp32 roundings)
 *   grad_lin[f, t]     = grad_lin[f, t]     + c_group * w[r]        (w: the 1-wide table with the same ids)
 * c_user / c_item / c_meta already contain the 1/B of the batch mean.  A row referenced n times in the batch receives
 * the term n times, once per staged reference; every staged row has one writer (no float atomics).  One launch covers
 * every reference of every group whose coefficient is not 0.  A group whose coefficient is exactly 0 is skipped
 * entirely: its fields are neither read nor written and its table is not gathered.  Linear has no 1-wide metadata
 * tables: those grad_lin fields are not touched.  Elements of the buffers beyond the F fields are not touched.
 * An id outside its table is not used as an address: its reference gets nothing added and bit 0 of *err_flag_dev (may
 * be NULL) is set.  B == 0, or every coefficient 0: TRS_OK, nothing launched.
 * TRS_E_ARG, nothing launched: tables NULL or a NULL member; net not TRS_NET_LINEAR / TRS_NET_FM; S outside 1..65;
 * M != tables->M; a D the scorer kernels do not take; a coefficient negative or not finite; grad_rows or grad_lin NULL;
 * NULL ids with B > 0; meta_dev NULL with M > 0 and c_meta > 0. */
int trs_stage_add_l2(int net, const trs_tables* tables, const int32_t* user_dev, const int32_t* items_dev,
                     const int32_t* meta_dev, int64_t B, int32_t S, int32_t M, float c_user, float c_item, float c_meta,
                     float* grad_rows_dev, float* grad_lin_dev, int32_t* err_flag_dev, void* stream);

/* ------------------------------------------------------------------ scorers: forward only (a2, a3, a6) */
/* Fused positive+negative scoring pass; the user row is gathered once for both passes.
 * net = TRS_NET_LINEAR: Linear.forward (collaborative/linear.py:54-80), score (B,1);
 * net = TRS_NET_FM:     FM.forward     (collaborative/fm.py:60-101),   score (B,) after sigmoid.
 * Replaces the two net.forward calls of TorchRecSys.forward (model.py:171-185).  neg_score may be NULL iff
 * batch->neg is NULL. */
int trs_score_forward(int net, const trs_tables* tables, const trs_batch* batch, float* pos_score_dev,
                      float* neg_score_dev, void* stream);

/* ------------------------------------------------- scorers: forward + hinge + backward (a2,a3,a5,a6,a7) */
/* One training pass over a batch with all rows read from the PRE-update tables (the semantics of
 * loss.backward() before optimizer.step(), model.py:188-200):
 *   scores as trs_score_forward; h = neg - pos + 1; loss_sum += sum max(h,0) (helper/loss.py:5-9; the caller divides
 *   by B); auc_count += #(pos > neg) (evaluate/metrics.py:23-31); per-triple gradient rows of d(mean hinge)/d(row)
 *   staged field-major into grad_rows (R,B,D) and the 1-wide terms into grad_lin (R,B) — i.e. exactly the
 *   uncoalesced values of the sparse COO gradients autograd builds (EmbeddingBackward), zero rows kept.
 * inv_B = 1/B of the mean.  pos_score/neg_score/auc_count may be NULL.  loss_sum/auc_count are ACCUMULATED
 * (atomic float / int adds): zero them before the first call. */
int trs_score_fwd_bwd(int net, const trs_tables* tables, const trs_batch* batch, float inv_B,
                      float* pos_score_dev, float* neg_score_dev, float* loss_sum_dev,
                      int32_t* auc_count_dev, float* grad_rows_dev, float* grad_lin_dev, int32_t loss, void* stream);

/* Backward only, from upstream d(loss)/d(score) (B,) per pass — the autograd.Function backward used when a caller
 * drives net.forward + its own loss (any objective), same staging as above. */
int trs_score_backward(int net, const trs_tables* tables, const trs_batch* batch, const float* gpos_dev,
                       const float* gneg_dev, float* grad_rows_dev, float* grad_lin_dev, void* stream);

/* ---------------------------------------------------------------- fused SGD training steps (a2,a3,a5-a9) */
/* n_steps whole training steps of a Linear / FM scorer WITHOUT metadata under plain SGD, driven from C (four kernel
 * launches per step, no host work in between) — the inner loop of TorchRecSys.fit (model.py:274-285) for
 * torch.optim.SGD(momentum=0, weight_decay=0).  Step s covers epoch positions [first_pos + s*batch, +batch).
 *   K1  forward + hinge + backward-to-scores at the PRE-update tables (software-pipelined row gathers); derives the
 *       batch from the resident stream (same shuffle / sampler as trs_batch_prepare, sample_offset = epoch position)
 *       when stream_ui (the stream as interleaved int32 pairs {user, item}, (N,2)) is non-NULL and writes it to user/pos/neg_buf (int32, (batch,)); otherwise reads the ids of
 *       step s from user/pos/neg_buf[s*batch ...] (an epoch slice prepared by the host: the bit-exact reference streams).  Stages gz (2,batch) and the user-row gradient du (batch,D);
 *       loss_sums[s] += sum of hinge terms.
 *   K2  item[pos] -= lr*gz+ * user[u], item[neg] -= lr*gz- * user[u] (+ 1-wide item terms) from the unmodified user rows:
 *       K2a the one reference per distinct row whose K1 ownership mark survived, by plain read-modify-write; K2b the
 *       remaining references of duplicated rows, by float atomics.  (One all-atomic launch when scratch is NULL.)
 *   K3  user[u] -= lr*du (+ 1-wide user term): plain for rows referenced once in the step, atomics for the others.
 * Same results as trs_score_fwd_bwd + trs_score_sgd_update (to summation order of duplicate rows).
 * That is the step's "marks" form.  The arguments select one of four forms, resolved once per call: marks; sorted item
 * references with marks for the users; sorted references with user-duplicate flags (adaptive rules, metadata); both
 * flag arrays without sorted references (flag mode) — see trs_train_args below and the head of csrc/fast_step.hip.
 * scratch: NULL or trs_train_scratch_bytes(n_users, n_items, batch, D) bytes, zero-initialised once; first_stamp: step counter
 * of the first step, non-zero, strictly increasing over the life of the scratch (re-zero the scratch before it wraps).
 * events: NULL, or 4*n_steps hipEvent_t handles recorded at the K1 | K2a+K2b | K3 boundaries of each step (a step whose handles are NULL is not timed) (bench.py). */
/* Update rule of the presorted two-launch step (opt == NULL: plain SGD with the lr argument).  The adaptive rules are
 * the ones the reference's users can actually run on its sparse embedding gradients:
 * torch.optim.SparseAdam (lazy Adam: rows present in the batch only) and torch.optim.Adagrad's sparse branch, applied
 * to the COALESCED gradient of each row — which the presorted runs provide: users referenced once are updated by K1,
 * duplicated users and item rows by their sorted runs; item runs cut at a 64-reference chunk boundary sum their pieces
 * in gacc and are applied by a small third launch.  State tables have the shapes of the weight tables and are updated
 * in place (the host mirror keeps them in optimizer.state[p], so optimizer.state_dict() stays truthful). */
#define TRS_OPT_SGD 0
#define TRS_OPT_SPARSE_ADAM 1
#define TRS_OPT_ADAGRAD 2
typedef struct trs_opt {
  int32_t kind;
  float lr, beta1, beta2, eps, lr_decay; /* read as the decimals they were written as: 1 - beta and each step's step
                                            size are formed in double from them, as torch does from its Python floats */
  int64_t step0;       /* optimiser step count before the first step of the call (same for the four tables) */
  float *user_s1, *user_s2, *item_s1, *item_s2;                 /* exp_avg | sum, exp_avg_sq | NULL        (n, D) */
  float *user_lin_s1, *user_lin_s2, *item_lin_s1, *item_lin_s2; /* the same for the 1-wide tables          (n, 1) */
  float* gacc;         /* (n_items, D) all-zero between steps: meeting point of the pieces of a cut item run */
  float* gacc_lin;     /* (n_items) */
  int32_t* cut_rows;   /* (cut_capacity) rows with a cut run in the current step */
  int32_t* cut_count;  /* [2] zero-initialised once; the steps alternate between the two counters */
  int32_t cut_capacity; /* >= 2*batch/64 + the number of rows with more than 64 references (2*batch is always enough) */
  /* Metadata scorers (tables->M > 0, trs_meta_stage with sorted columns): the same state per metadata column m < M.
   * meta_lin_* / meta_gacc_lin belong to the 1-wide metadata tables of FM; a Linear scorer has none and passes scratch
   * arrays of n_meta[m] floats.  meta_cut_rows[m]: cut_capacity entries; meta_cut_count[m]: [2], zeroed once. */
  float *meta_s1[TRS_MAX_META], *meta_s2[TRS_MAX_META], *meta_lin_s1[TRS_MAX_META], *meta_lin_s2[TRS_MAX_META];
  float *meta_gacc[TRS_MAX_META], *meta_gacc_lin[TRS_MAX_META];
  int32_t *meta_cut_rows[TRS_MAX_META], *meta_cut_count[TRS_MAX_META];
} trs_opt;
/* Metadata scorers (tables->M > 0) on the presorted step (plain SGD; the adaptive rules of trs_opt with sorted columns,
 * M <= 3 and D in {32, 64, 128, 256}): K1 is the generic scorer in a staging mode that
 * looks the metadata ids up in item_meta_tab, applies the user update in place, stages the rows the sorted item update
 * multiplies (FM: the per-pass field sums, Linear: the user row) and the metadata fields' gradients; user and item rows
 * then go through the sorted runs as without metadata, the (small, heavily shared) metadata tables through an atomic
 * scatter of the staged fields. */
typedef struct trs_meta_stage {
  const int32_t* item_meta_tab; /* (n_items, M) metadata ids of every item */
  float* xstage;                /* FM: (2, batch, D); Linear: (batch, D) */
  float* grad_rows;             /* (3 + 2M, batch, D): fields 3.. are written */
  float* grad_lin;              /* (3 + 2M, batch) */
  int32_t* meta_ids;            /* (2, batch, M) */
  /* Optional: every column's references sorted per batch (trs_epoch_presort_meta, offset to the call's first batch).
   * Then the metadata tables are updated by sorted runs like the item table (no gradient staging, no atomics but for
   * cut runs) and grad_rows / grad_lin / meta_ids may be NULL.  lin_scratch: max(n_meta) floats, used in place of the
   * 1-wide metadata tables a Linear scorer does not have. */
  const void* sorted_keys[TRS_MAX_META];
  const void* sorted_vals[TRS_MAX_META];
  float* lin_scratch;
  /* Optional: the slice's metadata ids by position, (n_steps * batch, M) int32 each, offset to the call's first batch
   * (written by trs_epoch_presort_meta): K1 reads them instead of looking them up behind the item ids. */
  const int32_t* pos_meta_ids;
  const int32_t* neg_meta_ids;
} trs_meta_stage;
/* Sorted references of metadata column m of an epoch slice whose ids exist (trs_epoch_presort): buffers and sizes as
 * trs_epoch_presort_sizes(n_batches, batch, n_cat, ...).  pos/neg_meta_out_dev (both or neither; (n_pos, M) int32): the
 * looked-up ids of column m, written for K1 (trs_meta_stage.pos_meta_ids / neg_meta_ids). */
int trs_epoch_presort_meta(const int32_t* pos_dev, const int32_t* neg_dev, int64_t n_batches, int64_t batch,
                           const int32_t* item_meta_dev, int32_t M, int32_t m, int64_t n_cat, void* keys_dev,
                           void* vals_dev, void* temp_dev, int64_t temp_bytes, int32_t* err_flag_dev,
                           void** sorted_keys_out, void** sorted_vals_out, int32_t* pos_meta_out_dev,
                           int32_t* neg_meta_out_dev, void* stream);
int64_t trs_train_scratch_bytes(int64_t n_users, int64_t n_items, int64_t batch, int32_t D);
/* Arguments of trs_train_steps_sgd (one struct instead of a 33-long positional list: a caller built against another
 * revision fails the trs_abi_version() check instead of shifting device pointers by one slot).  Zero-initialise, then
 * fill the groups that apply. */
typedef struct trs_train_args {
  int32_t net;               /* TRS_NET_LINEAR | TRS_NET_FM */
  int32_t n_steps;
  const trs_tables* tables;
  int64_t batch;
  float lr;                  /* plain SGD (opt == NULL) */
  int32_t loss;              /* TRS_LOSS_HINGE (0, the reference) | TRS_LOSS_BPR */
  uint32_t first_stamp;      /* with scratch: step counter of the first step, non-zero, strictly increasing */
  /* ids: derived from the resident stream (stream_ui != NULL; {user,item} int32 pairs, (N,2)) or given in the buffers */
  const int32_t* stream_ui_dev;
  const int32_t* neg_static_dev;
  int64_t N;
  uint64_t shuffle_key;
  uint64_t sample_seed;
  int64_t first_pos;
  int32_t* user_buf_dev;     /* (batch) outputs when derived; (n_steps*batch) inputs otherwise */
  int32_t* pos_buf_dev;
  int32_t* neg_buf_dev;
  /* staging and results */
  float* gz_buf_dev;         /* (2, batch) */
  float* du_buf_dev;         /* (batch, D) */
  float* loss_sums_dev;      /* (n_steps), accumulated */
  int32_t* err_flag_dev;
  void* scratch_dev;         /* NULL or trs_train_scratch_bytes(...) bytes, zeroed once */
  /* presorted two-launch step (trs_epoch_presort / trs_epoch_user_dups outputs, offset to the call's first batch) */
  const void* sorted_keys_dev;
  const void* sorted_vals_dev;
  int32_t key_bytes;         /* width of a sorted item key: 4 with sorted_keys_dev (what trs_epoch_presort_sizes reports),
                                0 without.  The sorted references carry 32-bit keys: 8 is refused (TRS_E_ARG). */
  int32_t ukey_bytes;        /* the same for sorted_ukeys_dev: 4 with the pairs (trs_epoch_user_dups), 0 without; 8 is
                                refused */
  const uint8_t* user_dup_flags_dev; /* (n_steps*batch) 1: the triple's user has another reference in its batch */
  const uint8_t* item_dup_flags_dev; /* (n_steps*batch, 2) NULL, or per triple {pos, neg}: 1 = the item row has another
                                        reference in the batch.  Given (plain SGD, no metadata): K1 also applies the
                                        item update of every reference that is ALONE on its row in place, and the
                                        sorted-run launch only walks rows referenced more than once.
                                        FLAG MODE (the sparse regime: most rows of a batch referenced once) = both flag
                                        arrays (trs_epoch_flags; they may be conservative), given ids, ustage, and NO
                                        sorted references: the flagged references follow K1 in a small second launch
                                        that adds their contributions into the tables with float atomics (all reads of
                                        the step happened in K1, so this is exact up to the order of those sums) */
  float* ustage_buf_dev;     /* (batch, D) */
  const void* sorted_ukeys_dev;
  const void* sorted_uvals_dev;
  int64_t slice_pos0;
  const trs_opt* opt;        /* NULL: plain SGD */
  const trs_meta_stage* meta;/* NULL iff tables->M == 0 */
  void** events;             /* NULL, or 4*n_steps hipEvent_t handles (a step whose handles are NULL is not timed) */
  uint32_t* sync_dev;        /* NULL, or TRS_SYNC_WORDS (288) uint32 in device memory (an arrival counter and eight flag
                                lines, 128 B apart), zeroed once by the caller, and */
  uint32_t* sync_count_host; /* ... ONE uint32 in HOST memory, zero at that time and owned by this entry point from
                                then on (the arrivals it has scheduled on sync_dev, mod 2^32).  FLAG MODE with both
                                given: whenever every workgroup of K1's grid is resident at once, the step is ONE
                                launch — K1's workgroups count themselves in on sync_dev[0] once their row reads are
                                done, wait for the whole grid, and add the flagged references' contributions
                                themselves (no second launch).  err bit 2: the grid did not become resident within
                                0.2 s (that step's results are not exact).  Before a step that finds the count at
                                TRS_SYNC_REBASE (2^30) or above, the entry point zeroes the TRS_SYNC_WORDS words on
                                the stream and the count with them: launches that count in early never write the
                                flag lines, and a line 2^31 arrivals old would read as "reached" (all launches on
                                one sync_dev therefore go to ONE stream). */
  const int32_t* n_flagged_dev; /* NULL, or (n_steps) int32 from trs_epoch_flags_ordered (the id and flag arrays above
                                then are the ones it ordered): batch st's first n_flagged_dev[st] triples are the ones
                                that carry a flagged reference.  The one-launch step then counts a workgroup in as soon
                                as it is past those triples and never waits for the slowest workgroup.  err bit 3: a
                                flagged reference was met behind those triples (arrays of another origin). */
} trs_train_args;
int trs_train_steps_sgd(const trs_train_args* args, void* stream);

/* Epoch-level grouping of the item references by row.  trs_epoch_presort covers n_batches whole batches starting at
 * epoch position first_pos: it writes the triples' ids (generated from the resident stream exactly as
 * trs_batch_prepare would, or taken as given when stream_ui is NULL) and the 2*batch references of every batch sorted
 * by item row (hand-written counting sort in LDS, one workgroup per batch; key = item row (uint32), payload = (t<<1)|which
 * (uint32), t = position inside the batch).  Passing the sorted arrays (offset to the first batch of the call) to
 * trs_train_steps_sgd together with the id arrays replaces K2a/K2b by one atomic-free launch: each run of equal keys is
 * summed by one lane group and applied with a plain whole-row read-modify-write (runs are cut every 64 references; cut
 * pieces of hot rows use float atomics).  Buffers: keys/vals two halves each (sizes from trs_epoch_presort_sizes).
 * item_dup_flags_out_dev (optional, 2*n_batches*batch bytes): byte 2q+w = 1 iff the item row of reference w (0 positive,
 * 1 negative) of position q is referenced again inside q's batch — neighbour compare on the sorted keys, scattered back
 * by payload (trs_train_args.item_dup_flags_dev). */
/* Per-position flags of an epoch slice: 1 iff the triple's user is referenced by another triple of the same batch
 * (per-batch counting sort of the user ids).  Passing them (offset to the first batch) with a (batch,D) staging buffer to
 * trs_train_steps_sgd in presorted mode lets K1 apply the user update itself for users referenced once in the batch
 * (plain store; K1 then stages the OLD user row for the item update instead of the gradient) — K3 shrinks to the
 * duplicated users: with the slice's sorted (user, position) pairs (offset to the call's first batch; slice_pos0 = that
 * batch's first position in the slice) each run of equal users is summed by one lane group and applied with one plain
 * read-modify-write.  The step then contains no float atomic except for cut runs of hot item rows. */
/* The sparse regime's whole presort in ONE launch, no sort: the ids of n_batches whole batches (generated as
 * trs_epoch_presort does, or taken as given) and per-reference duplicate flags — user_dup_flags (n_pos), item_dup_flags
 * (n_pos, 2) — found with a 2^20-bit bitmap in LDS, one 1024-thread workgroup per batch (set / re-set by the later
 * arrivals / test).  Tables with more rows than bits are hashed: the flags are then CONSERVATIVE (never 0 for a shared
 * row, possibly 1 for a lone one), which the flag mode of trs_train_steps_sgd tolerates.  Replaces the shuffle +
 * slicing + sampler loop of dataset/dataset.py:364-373,414-447 for the slice. */
int trs_epoch_flags(const int32_t* stream_ui_dev, const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key,
                    uint64_t sample_seed, int64_t first_pos, int64_t n_batches, int64_t batch, int64_t n_users,
                    int64_t n_items, int32_t* user_dev, int32_t* pos_dev, int32_t* neg_dev,
                    uint8_t* user_dup_flags_out_dev, uint8_t* item_dup_flags_out_dev, int32_t* err_flag_dev,
                    const trs_sampler* sampler, void* stream);
/* trs_epoch_flags, and — with n_flagged_out_dev (n_batches int32) — every batch partitioned IN PLACE (ids and flags
 * together; given ids are permuted too) so that the triples with at least one flagged reference come first; their
 * number goes to n_flagged_out_dev[b].  The order of the triples inside a batch means nothing to a training step (its
 * loss and gradients are sums over the batch): the same multiset of triples, the same flags per triple.  A batch with
 * more than 12 288 misplaced triples is left in its order and reported as n_flagged = batch.  Replaces nothing in the
 * reference (its order inside a batch is a random permutation too: FastDataLoader(shuffle=True), model.py:223-225). */
int trs_epoch_flags_ordered(const int32_t* stream_ui_dev, const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key,
                            uint64_t sample_seed, int64_t first_pos, int64_t n_batches, int64_t batch, int64_t n_users,
                            int64_t n_items, int32_t* user_dev, int32_t* pos_dev, int32_t* neg_dev,
                            uint8_t* user_dup_flags_out_dev, uint8_t* item_dup_flags_out_dev,
                            int32_t* n_flagged_out_dev, int32_t* err_flag_dev, const trs_sampler* sampler, void* stream);
/* User-duplicate flags alone, by the same LDS bitmap (no sort; conservative for n_users > 2^20).  Plain SGD without
 * metadata needs nothing else about the users: pass the flags to trs_train_steps_sgd with sorted_ukeys_dev = NULL and the
 * flagged users add their staged gradient rows with float atomics in the sorted-run launch. */
int trs_epoch_user_flags(const int32_t* user_dev, int64_t n_batches, int64_t batch, int64_t n_users,
                         uint8_t* flags_out_dev, void* stream);
int trs_epoch_user_dups_sizes(int64_t n_batches, int64_t batch, int64_t n_users, int64_t* ukeys_bytes_out,
                              int64_t* uvals_bytes_out, int64_t* temp_bytes_out);
int trs_epoch_user_dups(const int32_t* user_dev, int64_t n_batches, int64_t batch, int64_t n_users, void* ukeys_dev,
                        void* uvals_dev, void* temp_dev, int64_t temp_bytes, uint8_t* flags_out_dev,
                        void** sorted_ukeys_out, void** sorted_uvals_out, int32_t* ukey_bytes_out, void* stream);
/* Buffer sizes of trs_epoch_presort.  *key_bytes_out is always 4: keys are uint32 item rows, the only width
 * trs_train_steps_sgd takes (trs_train_args.key_bytes). */
int trs_epoch_presort_sizes(int64_t n_batches, int64_t batch, int64_t n_items, int64_t* key_bytes_out,
                            int64_t* keys_total_bytes_out, int64_t* vals_total_bytes_out, int64_t* temp_bytes_out);
int trs_epoch_presort(const int32_t* stream_ui_dev, const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key,
                      uint64_t sample_seed, int64_t first_pos, int64_t n_batches, int64_t batch, int64_t n_users,
                      int64_t n_items, int32_t* user_dev, int32_t* pos_dev, int32_t* neg_dev, void* keys_dev,
                      void* vals_dev, void* temp_dev, int64_t temp_bytes, int32_t* err_flag_dev,
                      void** sorted_keys_out, void** sorted_vals_out, uint8_t* item_dup_flags_out_dev,
                      const trs_sampler* sampler, void* stream);

/* ---------------------------------------------------------------- sparse row optimisers (a7, App. A.5) */
/* table[idx[t]] += alpha * vals[t]  for t < n, rows of D floats, vals row t at vals + t*ld.  Float atomics, one
 * 256-B segment per wave-instruction.  alpha = -lr is torch.optim.SGD's sparse param.add_(grad, alpha=-lr)
 * (third-party torch/optim/sgd.py, called from model.py:198).  Duplicate ids accumulate (uncoalesced COO). */
int trs_rows_scatter_add(float* table_dev, int64_t n_rows, int32_t D, const void* idx_dev, int32_t idx_bytes,
                         const float* vals_dev, int64_t ld, int64_t n, float alpha, int32_t* err_flag_dev,
                         void* stream);

/* Fused SGD update of every table of a scorer from the staging arrays of trs_score_fwd_bwd:
 * table_f[idx_f[t]] -= lr * grad_rows[f][t]  and the 1-wide tables likewise from grad_lin. */
int trs_score_sgd_update(int net, const trs_tables* tables, const trs_batch* batch, const float* grad_rows_dev,
                         const float* grad_lin_dev, float lr, void* stream);

/* Coalescing optimisers (SparseAdam / Adagrad / SGD-momentum need the per-row SUM of duplicates):
 *   1. trs_rows_scatter_add into `acc` (same shape as the table, all-zero between steps);
 *   2. trs_rows_apply_*: for every id in idx, the first arrival per distinct row (elected with atomicExch on
 *      stamp[row] == step_id) applies the update from acc[row] and clears acc[row].  Rows present in the batch are
 *      "touched" even when their gradient is zero.
 * step_id must be unique per (table, step) and never 0 after the stamps were zero-initialised. */
int trs_rows_apply_sparse_adam(float* table_dev, float* acc_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                               int32_t* stamp_dev, int64_t n_rows, int32_t D, const void* idx_dev,
                               int32_t idx_bytes, int64_t n, int32_t step_id, float lr, float beta1, float beta2,
                               float eps, int64_t step_count, void* stream);
int trs_rows_apply_adagrad(float* table_dev, float* acc_dev, float* state_sum_dev, int32_t* stamp_dev,
                           int64_t n_rows, int32_t D, const void* idx_dev, int32_t idx_bytes, int64_t n,
                           int32_t step_id, float clr, float eps, void* stream);

/* ------------------------------------------------------------------------------ hinge / AUC (a5, a12) */
/* loss_sum += sum_t max(neg-pos+1, 0); auc_count += #(pos > neg).  (helper/loss.py:5-9, evaluate/metrics.py:23-31)
 * loss = TRS_LOSS_BPR: the sum of softplus(neg - pos) instead (same for the two functions below). */
int trs_hinge_auc(const float* pos_dev, const float* neg_dev, int64_t B, float* loss_sum_dev,
                  int32_t* auc_count_dev, int32_t loss, void* stream);
/* The same for consecutive batches of `batch` rows of (n_total,) score arrays in one launch: loss_sums_dev[b] /
 * auc_counts_dev[b] (b < ceil(n_total / batch) <= 65535) accumulate batch b's sums — evaluate()'s per-batch metrics
 * (model.py:300-330) without one launch and one host round trip per batch. */
int trs_hinge_auc_batches(const float* pos_dev, const float* neg_dev, int64_t n_total, int64_t batch,
                          float* loss_sums_dev, int32_t* auc_counts_dev, int32_t loss, void* stream);
/* d(mean hinge)/d(pos), d(.)/d(neg): -a/B, +a/B with a = [neg-pos+1 >= 0] (torch clamp subgradient). */
int trs_hinge_backward(const float* pos_dev, const float* neg_dev, int64_t B, float inv_B, float* gpos_dev,
                       float* gneg_dev, int32_t loss, void* stream);
/* trs_hinge_auc and trs_hinge_backward in one sweep over the scores (the MLP training step; the sums are formed in
 * trs_hinge_auc's order, the gradients are trs_hinge_backward's).  loss_sum_dev / auc_count_dev may be NULL. */
int trs_hinge_auc_backward(const float* pos_dev, const float* neg_dev, int64_t B, float inv_B, float* loss_sum_dev,
                           int32_t* auc_count_dev, float* gpos_dev, float* gneg_dev, int32_t loss, void* stream);

/* ---------------------------------------------------------------------------------- predict (a13) */
/* Scores of ONE user against items [item0, item0+n) (model.py:341-452: net.forward over item chunks, pos keys
 * only).  item_meta (n_items,M) int32 gives each item's metadata ids (NULL when M == 0). */
int trs_score_all_items(int net, const trs_tables* tables, int64_t user_id, int64_t item0, int64_t n,
                        const int32_t* item_meta_dev, float* score_out_dev, void* stream);
/* Top-k of scores (n,) by (score descending, index ascending) -> idx_out (k,) int64, any 1 <= k <= n.  workspace: at
 * least trs_topk_workspace_bytes(n, k) bytes.  (torch.sort(descending=True)[:top_k], model.py:447-450)
 * k <= 2048: per-chunk bitonic selection (4096 keys in LDS, iterated); larger k: a full bitonic sort of the padded keys
 * in global memory (the reference sorts all scores for any top_k). */
int64_t trs_topk_workspace_bytes(int64_t n, int32_t k);
int trs_topk(const float* scores_dev, int64_t n, int32_t k, int64_t* idx_out_dev, void* workspace_dev,
             int64_t workspace_bytes, void* stream);


/* ------------------------------------------------------------------------------------- retrieval (recommend) */
/* Batched top-k of Linear / FM scores over the whole catalogue (model.py recommend / evaluate_ranking, DESIGN.md
 * "Retrieval").  For one user both scorers are an inner product plus constants:
 *   Linear  score(u,i) = (<U_u, S_i> + user_bias_u) + c_i,  c_i = item_bias_i
 *   FM      z(u,i)     = (<U_u, S_i> + linear_user_u) + c_i,
 *           c_i = linear_item_i + sum_m linear_meta_m + 1/2 (|S_i|^2 - |item_i|^2 - sum_m |meta_m|^2),  score = sigmoid(z)
 * with S_i = item_i + sum_m meta_m (the item's row plus the rows of its metadata).  Items are ranked by the raw Linear
 * score and by z for FM (strict where fp32 sigmoid saturates), ties by ascending item id. */
#define TRS_RETRIEVE_KMAX 128 /* largest k of the fused kernel (its per-user LDS candidate buffer holds KMAX + 128) */
#define TRS_RETRIEVE_DMAX 256 /* largest D of the fused kernel */

/* Rows of a sorted CSR indexed by dense user id: items of row u are items[off[u] .. off[u+1]), ascending. */
typedef struct trs_csr {
  const int64_t* off;   /* (n_rows + 1) */
  const int32_t* items; /* (off[n_rows]) */
  int64_t n_rows;
} trs_csr;

/* Bytes of the folded item buffer of a catalogue of n_items items with D factors (0 when D > TRS_RETRIEVE_DMAX): the
 * item matrix S (n_items rounded up to 128 rows, D zero-padded to 16/32/64/128/256 columns) then c (same rows). */
int64_t trs_item_fold_bytes(int64_t n_items, int32_t D);
/* S and c of every item (formulas above) into fold_dev; item_meta (n_items, M) int32 gives each item's metadata ids
 * (NULL when M == 0).  Padding rows are zero. */
int trs_item_fold(int net, const trs_tables* tables, const int32_t* item_meta_dev, void* fold_dev, int64_t fold_bytes,
                  void* stream);
/* Workspace of trs_retrieve_topk for n_q query users and k (per-split partial top-k lists); monotone in n_q and k. */
int64_t trs_retrieve_workspace_bytes(int64_t n_q, int32_t k);
/* Top-k items of each query user users[q] (dense ids, int64), 1 <= k <= min(TRS_RETRIEVE_KMAX, n_items), from the
 * folded buffer trs_item_fold wrote for the same tables.  seen (optional): the users' items to exclude.  Outputs
 * ids (n_q, k) int64 and scores (n_q, k) fp32 in the scorer's output units (FM: sigmoid(z)); positions beyond the
 * user's count of candidate items hold id -1 and score -inf.  rel (optional): the users' relevant items; metrics_out
 * (n_q, 4) float64 = (hits, dcg, idcg, n_rel) of the returned list (trs_rank_metrics).  One fp32 MFMA kernel streams
 * item tiles past a tile of 32 users with the top-k selection fused; a merge kernel joins the item splits. */
int trs_retrieve_topk(int net, const trs_tables* tables, const void* fold_dev, int64_t fold_bytes,
                      const int64_t* users_dev, int64_t n_q, int32_t k, const trs_csr* seen, const trs_csr* rel,
                      int64_t* ids_out_dev, float* scores_out_dev, double* metrics_out_dev, void* workspace_dev,
                      int64_t workspace_bytes, void* stream);
/* Score rows (n_rows, n_items) fp32: row r's entries at the seen items of user users[r] become -inf (the lowest value
 * trs_topk ranks; callers pad the positions beyond n_items - |seen_u| with -1).  Generic retrieval path (MLP, k > KMAX). */
int trs_mask_seen(float* scores_dev, int64_t n_rows, int64_t n_items, const int64_t* users_dev, const trs_csr* seen,
                  void* stream);
/* Ranking metrics of given top-k lists ids (n_q, k) int64 (-1 = no item) against the relevant items rel of users[q]:
 * metrics_out (n_q, 4) float64 = (hits = |R_u & T_u|, dcg = sum_{r<k, R_u[r] in T_u} 1/log2(r+2),
 * idcg = sum_{r<min(k,|T_u|)} 1/log2(r+2), n_rel = |T_u|), sums in ascending r. */
int trs_rank_metrics(const int64_t* ids_dev, int64_t n_q, int32_t k, const int64_t* users_dev, const trs_csr* rel,
                     double* metrics_out_dev, void* stream);

/* ------------------------------------------------------------------------------------------- sequence model */
/* A factorised Markov model over the last L items of a user's ORDERED history (model.py fit_sequence, DESIGN.md 4.18;
 * FPMC for L = 1, the Fossil family for L > 1; the reference names a sequence model as "yet to come" and has none, so
 * this contract, not a reference output, pins it).  Added without touching an existing signature or struct.
 * Tables: the Linear scorer's U = tables->user (n_users, D), V = tables->item (n_items, D), b = tables->item_lin
 * (n_items, 1), without metadata (tables->M == 0), plus the context table C = ctx (n_items, D).  Fixed weights
 * w_0 .. w_{L-1} (ctx_weight, L floats on the device); l = 0 is the most recent item.
 * Sequences: a trs_csr whose rows are NOT sorted: items[off[u] .. off[u+1]) is user u's sequence s_u, oldest first,
 * repeated items kept.  For position k of s_u slot l is present iff l < k (absent slots are always the oldest ones):
 *   q(u, k)   = U[u] + sum_{l < min(L, k)} w_l * C[s_u[k-1-l]]     added in the order l = 0, 1, ...: per element the
 *               product, then the sum, two fp32 roundings; an absent slot adds nothing (q keeps its bits)
 *   z(u,k,i)  = <q(u, k), V[i]> + b[i]     (per lane the products of its columns summed in ascending column order from
 *               0, the lanes of the group by the xor butterfly: trs_score_fwd_bwd's inner product, on q)
 *   row loss  = pair(z(u,k,p), z(u,k,n)), p = s_u[k], n the given negative: trs_score_fwd_bwd's pair loss (hinge =
 *               max(0, z_n - z_p + 1), bpr = -log sigmoid(z_p - z_n)).
 * With gp = d loss / d z_p * inv_B and gn = -gp:  dU[u] = gp V[p] + gn V[n],  dV[p] = gp q,  dV[n] = gn q,  db[p] = gp,
 * db[n] = gn,  dC[s_u[k-1-l]] = w_l * dU[u] for every present slot.  All rows are read from the PRE-update tables.  The
 * user's 1-wide table (tables->user_lin) takes no part: it enters both z alike and its gradient is 0.  With C = 0 or
 * L = 0 the staged user / item fields, grad_lin and the loss are trs_score_fwd_bwd(TRS_NET_LINEAR)'s on the same (user,
 * positive, negative) with a zero user_lin, bit for bit. */
#define TRS_SEQ_LMAX 16 /* largest context length L */
/* trs_seq_fwd_bwd: one training pass over B triples (user[t], entry[t], neg[t]): entry[t] (int64) is a position in the
 * CSR's item array, from which the kernel derives k = entry - off[user], p = items[entry] and the context ids
 * items[entry-1-l] — no (N, L) context array exists.  loss_sum += the sum of the row losses (the caller divides by B);
 * auc_count (may be NULL) += #(z_p > z_n).  Both are ACCUMULATED.  inv_B = 1/B of the mean.
 * Staged gradients, field-major: grad_rows (3 + L, B, D) and grad_lin (3, B); field 0 the user, 1 the positive, 2 the
 * negative (trs_score_fwd_bwd's order), field 3 + l context slot l.  ctx_ids_out (L, B) int32: the row of C each slot's
 * gradient belongs to.  An absent slot gets id 0 and an all-zero gradient row, so a scatter adds -lr * 0 to row 0.
 * grad_rows == NULL (then grad_lin must be NULL too): forward only — the same loss and AUC count, nothing staged.
 * A user outside [0, min(n_users, seq->n_rows)), a negative, positive or present context id outside [0, n_items), or an
 * entry outside its user's range [off[user], off[user+1]) is clamped for addressing, sets bit 0 of *err_flag_dev (may be
 * NULL) and zeroes its row's loss and gradients.
 * TRS_E_ARG, nothing launched: tables NULL or a NULL member (user, item and both 1-wide tables); tables->M != 0; a D the
 * scorer kernels do not take; ctx NULL; seq NULL, without offsets or item ids, or with no rows; L outside
 * 0..TRS_SEQ_LMAX; ctx_weight NULL with L > 0; a loss id other than TRS_LOSS_HINGE / TRS_LOSS_BPR; loss_sum NULL;
 * grad_lin without grad_rows or the reverse; ctx_ids_out NULL while gradients of L > 0 slots are staged; B < 0; NULL
 * ids with B > 0. */
int trs_seq_fwd_bwd(const trs_tables* tables, const float* ctx_dev, const trs_csr* seq, const int32_t* user_dev,
                    const int64_t* entry_dev, const int32_t* neg_dev, int64_t B, int32_t L,
                    const float* ctx_weight_dev, int32_t loss, float inv_B, float* loss_sum_dev,
                    int32_t* auc_count_dev, float* grad_rows_dev, float* grad_lin_dev, int32_t* ctx_ids_out_dev,
                    int32_t* err_flag_dev, void* stream);
/* trs_seq_user_rows: query rows for retrieval.  seq has one row per output row (seq->n_rows == n), oldest first; for
 * r < n, with len = the row's length:
 *   out[r*ld .. r*ld + D) = (U[users[r]], or 0 when users[r] < 0 or users_dev is NULL) + sum_{l < min(L, len)} w_l *
 *   C[row r's item len-1-l], in the order and roundings of q above (l = 0, the row's LAST item, first).
 * ld >= D floats is the caller's row stride (a multiple of 4 when D is); columns D .. ld-1 are not written.  No bias: b
 * stays with the item side.  One launch, one writer per row, no atomics: a float32 loop on the host reproduces the rows
 * bit for bit.  A user >= n_users or a context id outside [0, n_items) sets bit 0 of *err_flag_dev (may be NULL) and
 * zeroes the row.
 * TRS_E_ARG, nothing launched: the table, context, CSR, L and ctx_weight grounds of trs_seq_fwd_bwd (item ids may be
 * NULL only with L == 0: the host cannot see that every row is empty, so a caller without any id passes a one-element
 * buffer, which is never read); seq->n_rows != n; n < 0; ld < D, or not a multiple of 4 with D % 4 == 0; out NULL with n > 0. */
int trs_seq_user_rows(const trs_tables* tables, const float* ctx_dev, const trs_csr* seq, const int64_t* users_dev,
                      int64_t n, int32_t L, const float* ctx_weight_dev, float* out_dev, int64_t ld,
                      int32_t* err_flag_dev, void* stream);

/* ------------------------------------------------------------------- nearest neighbours (similar_items / _users) */
/* Neighbour search over the rows of one table (model.py similar_items / similar_users): the similarity
 * of rows q and j is <x_q, x_j> (dot) or <x^_q, x^_j> with x^ = x * (1 / |x|) (cosine: normalise first, then the fp32
 * inner product; a zero row has x^ = 0).  Added without touching an existing signature or struct.
 *
 * trs_neighbour_fold: rows (n_rows, D) fp32 with row stride ld >= D floats (the S block of a trs_item_fold buffer with
 * ld = its padded width, or a user table with ld = D) -> fold_dev in trs_item_fold's layout, trs_item_fold_bytes(n_rows,
 * D) bytes: X^ (n_rows rounded up to 128 rows, D zero-padded to 16/32/64/128/256 columns; padding rows and columns are
 * zero), then as many zeros as rows where trs_item_fold keeps c.  cosine = 0 copies and pads; cosine = 1 multiplies each
 * row by its inverse norm: per lane l of one wave the squares of columns 4l .. 4l+3 summed in ascending column order
 * (fp32, product and sum rounded separately, from 0), the 64 lane sums added by the xor butterfly of strides 32, 16, 8,
 * 4, 2, 1, then 1.0f / sqrtf(sum), or 0 when the sum is 0.  fold_dev must not overlap rows_dev. */
int trs_neighbour_fold(const float* rows_dev, int64_t n_rows, int32_t D, int64_t ld, int32_t cosine, void* fold_dev,
                       int64_t fold_bytes, void* stream);
/* Top-k neighbours of the rows queries[q] (dense row ids, int64) among the n_rows rows of a trs_neighbour_fold buffer,
 * 1 <= k <= min(TRS_RETRIEVE_KMAX, n_rows): the fused kernel of trs_retrieve_topk with the buffer as both operands, all
 * constants zero and each query's own row excluded (another row with identical values is not).  Outputs ids (n_q, k)
 * int64 and the raw inner products (n_q, k) fp32, by (similarity descending, row id ascending); positions beyond the
 * n_rows - 1 candidates hold id -1 and score -inf, and so does the whole row of a query outside [0, n_rows), which is
 * never used as an address (trs_retrieve_topk treats a user outside its table the same way).  workspace: at least
 * trs_retrieve_workspace_bytes(n_q, k) bytes. */
int trs_neighbours_topk(const void* fold_dev, int64_t fold_bytes, int64_t n_rows, int32_t D,
                        const int64_t* queries_dev, int64_t n_q, int32_t k, int64_t* ids_out_dev,
                        float* scores_out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* --------------------------------------------------------- fold-in of unseen users (fold_in_users) */
/* One new user row per item history, the item side frozen: E epochs of per-visit SGD on z(u,i) = (<u, S_i> + b) + c_i,
 * S and c those of a trs_item_fold buffer of (n_items, D) (layout unchanged, read only).  One launch for all users.
 * Added without touching an existing signature or struct.
 * hist: CSR of the n_new = hist->n_rows new users, off int64 (n_new + 1), items int32; every row holds sorted, distinct
 * dense item rows; n_h = off[h+1] - off[h].  State per user h: u in R^D = 0, b = 0, fp32.
 * For epoch e = 0 .. E-1, visit j = 0 .. n_h-1, in this order, sequentially:
 *   order      r = j when shuffle == 0, else r = trs_feistel_perm(j, n_h, key_e, trs_feistel_half_bits(n_h)), key_e =
 *              ((y << 32) | x) | 1 of trs_philox4x32_10(counter = e, key = (seed + 0xD1B54A32D192ED03) mod 2^64);
 *              p = items[off[h] + r].
 *   negative   n = trs_sample_neg_opt(seed, ctr = ((uint64)e << 32) | r, u = h, pos = p, n_items, sampler): max_tries
 *              candidates, one rejected while the history holds it (the seen CSR is the history CSR itself) when
 *              reject_seen; the last candidate is kept whatever it is, as in training.  Without reject_seen every
 *              max_tries gives the plain draw trs_sample_one_neg (max_tries = 0 calls it).  No popularity option.
 *   purity     the schedule depends on (seed, e, r, n_h) and the history only, not on h or on what else is in the call:
 *              a history folds in to the same row alone or among 10 000 others.
 *   scores     z_p = (sum_d u_d * S_{p,d} + b) + c_p, z_n likewise; s = z (Linear), s = sigmoid(z) (FM).  The order of
 *              the sum over d is the kernel's (per lane four ascending columns, then trs_group_sum).
 *   loss       (value, dneg) = trs_pair_loss(loss, s_p, s_n), loss = TRS_LOSS_HINGE (active at h >= 0) | TRS_LOSS_BPR.
 *   gradients  g_p = -dneg * w_p, g_n = dneg * w_n; w = 1 (Linear), w = s (1 - s) (FM).
 *   update     u_d <- u_d - lr * ((g_p * S_{p,d} + g_n * S_{n,d}) + l2 * u_d);  b <- b - lr * ((g_p + g_n) + l2 * b)
 *              (Linear: g_p + g_n = 0, so with l2 = 0 the bias stays exactly 0); every product and sum rounded to fp32.
 *   loss_out   loss_out[e][h] = (sum of the epoch's values in visit order) / n_h; 0 for an empty history.
 * An item id outside [0, n_items) is never used as an address: that visit is skipped (no update, nothing added to the
 * loss sum) and bit 0 of *err_flag_dev (may be NULL) is set.
 * Outputs: user_out (n_new, D), user_lin_out (n_new), loss_out (epochs, n_new) or NULL; each written once.
 * TRS_E_ARG, nothing launched: net not TRS_NET_LINEAR / TRS_NET_FM; D outside 1..TRS_RETRIEVE_DMAX; n_items < 2 (or
 * >= 2^31); fold_dev NULL or fold_bytes < trs_item_fold_bytes(n_items, D); loss not hinge / BPR; epochs outside
 * 1..1024; lr not finite or <= 0; l2 not finite or < 0; max_tries outside 0..64; reject_seen with max_tries == 0; hist
 * NULL; with n_new > 0 a NULL array of hist or a NULL user_out / user_lin_out.  n_new == 0: TRS_OK, nothing launched. */
int trs_fold_in_users(int net, const void* fold_dev, int64_t fold_bytes, int64_t n_items, int32_t D,
                      const trs_csr* hist, int32_t loss, int32_t epochs, float lr, float l2, uint64_t seed,
                      int32_t shuffle, int32_t reject_seen, int32_t max_tries, float* user_out_dev,
                      float* user_lin_out_dev, float* loss_out_dev, int32_t* err_flag_dev, void* stream);

/* ------------------------------------------------------ item fold-in of unseen items (fold_in_items) */
/* One new item row per user history, everything else frozen: E epochs of per-visit SGD on the item's own row v and its
 * 1-wide entry beta.  One launch for all items.  Added without touching an existing signature or struct.
 * Frozen inputs: the user table U (n_users, D) = tables->user (unpadded, row stride D) with a = tables->user_lin
 * (n_users); the catalogue's fold (S, c) = fold_dev, a trs_item_fold buffer of (n_items, D); the train interactions
 * (stream_user, stream_item), n_stream rows, int32, dense ids; seen (optional): the model's seen CSR, user -> sorted
 * train items.  Of `tables` only user, user_lin, n_users and D are read.
 * Per new item h: hist row h = its sorted, distinct dense user ids (off int64 (n_new + 1), items int32 hold the users;
 * n_h = off[h+1] - off[h]); its metadata part T_h in R^Dp and kappa_h = row h of S and c of new_fold_dev, a trs_item_fold
 * buffer of (n_new, D) written for a table set whose item rows and 1-wide item rows are zero and whose metadata ids are
 * the new items' (so T = sum_m meta_m, kappa = the c of an item with a zero row; M == 0: both 0).
 * State per item h: v in R^D = 0, beta = 0, fp32.  With x_d = v_d + T_d (one rounding):
 *   z_new(u)   = ((sum_d U[u,d] * x_d) + a_u) + c_new,   c_new = beta + kappa (Linear) | (beta + kappa) + sum_d v_d * T_d (FM)
 *   z_old(u,o) = ((sum_d U[u,d] * S[o,d]) + a_u) + c_o
 *   s = z (Linear) | sigmoid(z) = 1 / (1 + expf(-z)) (FM);  w(s) = 1 | s (1 - s);  dir_d = U[u,d] | U[u,d] + T_d
 *   sums       every sum over d is the kernel's: per lane of the item's group of Dp / 4 lanes the four products of
 *              columns 4l .. 4l+3 added in ascending column order from the first product, then trs_group_sum (the xor
 *              butterfly of strides Dp/8 .. 1); columns >= D of U read as 0.
 * For epoch e = 0 .. E-1, visit j = 0 .. n_h * (1 + nu) - 1 (nu = negative_visits), in this order, sequentially:
 *   order      q = j / (1 + nu), t = j mod (1 + nu); r = q when shuffle == 0, else r = trs_feistel_perm(q, n_h, key_e,
 *              trs_feistel_half_bits(n_h)), key_e that of "fold-in" above.  ctr = ((uint64)e << 32) | r.
 *   t == 0     the new item is the positive: u = items[off[h] + r];
 *              o = trs_sample_neg_opt(seed, ctr, u, pos = n_items, n_items + 1, sampler): the new item stands for row
 *              n_items of a catalogue one longer, so o is uniform over [0, n_items); with reject_seen and seen != NULL a
 *              candidate that seen row u holds is redrawn, at most max_tries candidates, the last kept (seen == NULL
 *              or reject_seen == 0: the first candidate; max_tries == 0 calls trs_sample_one_neg).
 *              (value, dneg) = trs_pair_loss(loss, s(z_new(u)), s(z_old(u,o)));  g = -dneg * w(s_new).
 *   t >= 1     the new item is the negative of a train interaction: candidate k = 0, 1, .. is row
 *              idx_k = mulhi64((y << 32) | x, n_stream) of trs_philox4x32_10(counter = ctr, key = (seed +
 *              (1 + t) * 0xD1B54A32D192ED03 + k * 0x9E3779B97F4A7C15) mod 2^64); with reject_seen a candidate whose user
 *              stream_user[idx_k] is in history row h (binary search) is redrawn, at most max_tries candidates, the
 *              last kept; without, candidate 0.  (u, o) = (stream_user[idx], stream_item[idx]).
 *              (value, dneg) = trs_pair_loss(loss, s(z_old(u,o)), s(z_new(u)));  g = +dneg * w(s_new).
 *   update     v_d <- v_d - lr * ((g * dir_d) + l2 * v_d);  beta <- beta - lr * (g + l2 * beta); every product and sum
 *              rounded to fp32.
 *   loss_out   loss_out[e][h] = (sum of the epoch's values in visit order) / (float)(n_h * (1 + nu)); 0 for n_h == 0.
 *   purity     the result for an item depends on its history, T_h, kappa_h, the options and the frozen inputs only, not
 *              on h or on the other items of the call.  n_h == 0 gives v = 0, beta = 0: the metadata-only item.
 * A user id outside [0, n_users) or a stream item outside [0, n_items) is never used as an address: that visit is
 * skipped (no update, nothing added to the loss sum) and bit 0 of *err_flag_dev (may be NULL) is set.
 * Outputs: item_out (n_new, D), item_lin_out (n_new), loss_out (epochs, n_new) or NULL; each written once.
 * TRS_E_ARG, nothing launched: what trs_fold_in_users rejects (net, D, n_items, fold buffer, loss, epochs, lr, l2,
 * max_tries, reject_seen with max_tries == 0, hist NULL, FOLDIN_DEPTH; with n_new > 0 a NULL array of hist or a NULL
 * output), with D = tables->D, and n_items == 2^31-1 (row n_items must be an int32 too); tables NULL, a NULL user /
 * user_lin table, n_users outside 1..2^31-1; negative_visits outside 0..8; negative_visits > 0 with n_stream <= 0 or a NULL stream; n_stream < 0; with n_new > 0
 * new_fold_dev NULL or new_fold_bytes < trs_item_fold_bytes(n_new, D); seen with a NULL array.  n_new == 0: TRS_OK,
 * nothing launched. */
int trs_fold_in_items(int net, const trs_tables* tables, const void* fold_dev, int64_t fold_bytes, int64_t n_items,
                      const void* new_fold_dev, int64_t new_fold_bytes, const trs_csr* hist,
                      const int32_t* stream_user_dev, const int32_t* stream_item_dev, int64_t n_stream,
                      const trs_csr* seen, int32_t loss, int32_t epochs, float lr, float l2, int32_t negative_visits,
                      uint64_t seed, int32_t shuffle, int32_t reject_seen, int32_t max_tries, float* item_out_dev,
                      float* item_lin_out_dev, float* loss_out_dev, int32_t* err_flag_dev, void* stream);

/* ------------------------------------------------------------------- implicit ALS (fit_als) */
/* Weighted alternating least squares on implicit feedback (Hu, Koren, Volinsky, ICDM 2008): preference 1 with confidence
 * 1 + alpha on the observed pairs, preference 0 with confidence 1 everywhere else.  One half-sweep re-solves every row of
 * one table with the other table frozen: trs_als_gram once, then trs_als_solve once, for all rows.  Added without
 * touching an existing signature or struct.
 *
 * trs_als_gram: G (D, D) = Y^T Y in fp32 of the first n rows and D columns of rows (row stride ld >= D floats).
 *   Deterministic: the rows are cut into chunks of R = max(16, ceil(ceil(n / C) / 16) * 16) rows, C = 512 (D <= 128) |
 *   256 (D > 128); the partial sum of a chunk is one fmaf chain per entry over the chunk's rows in ascending order, from
 *   0; G[a][b] is the sum of the chunks' partials in ascending chunk order, from 0.  No atomics: the same input gives
 *   the same bits, and G[a][b] == G[b][a].  workspace: trs_als_gram_workspace_bytes(n, D) = ceil(n / R) * D * D * 4
 *   bytes.  n == 0 writes G = 0.
 *   TRS_E_ARG, nothing launched: D outside 1..TRS_RETRIEVE_DMAX; n < 0 (or >= 2^31); ld < D; G_out NULL; with n > 0 a NULL
 *   rows or workspace.
 *
 * trs_als_solve: Y = other_rows (n_other, D, row stride D) frozen, G (D, D, row stride D) as trs_als_gram wrote it for
 *   Y, nbr the CSR of the n_rows rows to solve (off int64 (n_rows + 1), items int32: sorted, distinct rows of Y),
 *   rows_inout (n_rows, D, row stride D) the start values, overwritten by the results.  One launch.  Per row h with
 *   neighbour list N = items[off[h] .. off[h+1]):
 *     |N| == 0   the row is set to exactly 0.
 *     otherwise  at most cg_steps steps of conjugate gradient on A x = b from the row's current value x,
 *                  A = G + lambda I + alpha sum_{i in N} y_i y_i^T,   b = (1 + alpha) sum_{i in N} y_i,
 *                A never formed (the recurrence of the `implicit` package's GPU solver):
 *                  A v   = ((G v)_d + lambda * v_d) + alpha * acc_d,  acc = sum_{i in N} (y_i . v) y_i
 *                  b_d   = (1.0f + alpha) * s_d,  s = sum_{i in N} y_i
 *                  r = b - A x;  p = r;  rho = r . r;  stop if rho < 1e-20
 *                  per step:  a = rho / (p . A p);  x += a p;  r -= a A p;  rho' = r . r;  stop if rho' < 1e-20;
 *                             p = r + (rho' / rho) p;  rho = rho'
 *   sums       every product and sum is rounded to fp32 on its own (no fused multiply-add).  acc and s run over the
 *              neighbours in CSR order, from 0.  (G v)_d = sum_e G[e][d] * v_e for e ascending, from 0 (row e of G is
 *              read).  The order of a sum over d (y . v, r . r, p . A p) is the kernel's: per lane of the row's group of
 *              Dp / 4 lanes (Dp = D rounded up to a power of two >= 16) the four products of columns 4l .. 4l+3 added in
 *              ascending column order from the first product, then trs_group_sum (the xor butterfly of strides Dp/8 .. 1);
 *              columns >= D count as 0.
 *   purity     a row's result depends on its own list, its start value, Y, G, lambda, alpha and cg_steps only: not on h,
 *              not on the other rows of the call.
 * A neighbour id outside [0, n_other) is never used as an address: that neighbour is skipped (in acc and in s) and bit
 * 0 of *err_flag_dev (may be NULL) is set.
 * TRS_E_ARG, nothing launched: D outside 1..TRS_RETRIEVE_DMAX; cg_steps outside 1..256; lambda not finite or <= 0; alpha
 * not finite or < 0; n_rows < 0; with n_rows > 0 n_other outside 1..2^31-1, a NULL other_rows / G / rows_inout, nbr NULL
 * or with a NULL array, nbr->n_rows != n_rows.  n_rows == 0: TRS_OK, nothing launched. */
int64_t trs_als_gram_workspace_bytes(int64_t n, int32_t D);
int trs_als_gram(const float* rows_dev, int64_t n, int32_t D, int64_t ld, float* G_out_dev, void* workspace_dev,
                 void* stream);
int trs_als_solve(const float* other_rows_dev, int64_t n_other, int32_t D, const float* G_dev, const trs_csr* nbr,
                  float lambda, float alpha, int32_t cg_steps, float* rows_inout_dev, int64_t n_rows,
                  int32_t* err_flag_dev, void* stream);

/* ------------------------------------------------------------------- LightGCN (fit_lightgcn) */
/* LightGCN (He et al., SIGIR 2020) on the train split's distinct (user, item) pairs: with A^ the symmetric normalised
 * bipartite adjacency, A^[u][i] = dinv_u * dinv_i on a pair (dinv = 1 / sqrt(degree), 0 for degree 0), and E0 = [U0; V0]
 * the base tables,  Final = 1/(K+1) * sum_{k=0..K} A^^k E0,  score = <Final_u, Final_i>.  The sum is evaluated in Horner
 * form, F_K = E0, F_k = E0 + A^ F_{k+1}, Final = 1/(K+1) * F_0; the gradient of a loss with G = dL/dFinal is the same
 * recurrence on G (A^ is symmetric).  One Horner step is two calls of trs_lgcn_propagate: user rows from item rows
 * through the by-user CSR, item rows from user rows through the by-item CSR.  Added without touching an existing
 * signature or struct.
 *
 * trs_lgcn_propagate: in_rows (n_in, D, row stride D); nbr the CSR of the n_out rows to write (off int64 (n_out + 1),
 *   items int32: rows of in_rows); dinv_out (n_out), dinv_in (n_in); add_rows (n_out, D, row stride D) or NULL; out_rows
 *   (n_out, D, row stride D).  One launch.  For row r with list N = items[off[r] .. off[r+1]) and column d:
 *     segments   N is cut into segments of TRS_LGCN_SEG neighbours in CSR order; the last may be shorter.
 *     partial_j  = sum over segment j's neighbours c, in CSR order, from 0, of  dinv_in[c] * in[c][d]
 *     s          = the sum of the partials in ascending segment order, from 0 (a list of at most TRS_LGCN_SEG
 *                  neighbours is therefore one straight sum; an empty list has s = 0)
 *     p          = dinv_out[r] * s
 *     v          = scale * (add_rows ? add_rows[r][d] + p : p)
 *     out[r][d]  = accumulate ? out[r][d] + v : v          (every row is written, also one with an empty list)
 *   sums       every product and every sum is rounded to fp32 on its own (no fused multiply-add): a float32 loop on the
 *              host reproduces the rows bit for bit, whatever the launch shape.
 *   purity     a row's result depends on its own list, its add / out / dinv_out value, the rows it names (with their
 *              dinv_in) and scale only: not on r, not on the other rows of the call.
 *   aliasing   out_rows may be add_rows.  out_rows == in_rows is TRS_E_ARG.
 * A neighbour id outside [0, n_in) is never used as an address (into in_rows or dinv_in): that neighbour is skipped (it
 * keeps its place in its segment) and bit 0 of *err_flag_dev (may be NULL) is set.
 * TRS_E_ARG, nothing launched: D outside 1..TRS_RETRIEVE_DMAX; scale not finite; accumulate outside {0, 1}; n_out < 0 or
 * n_in < 0; nbr NULL or nbr->n_rows != n_out; with n_out > 0 a NULL in_rows / dinv_out / dinv_in / out_rows or CSR array,
 * or n_in outside 1..2^31-1.  n_out == 0: TRS_OK, nothing launched.
 *
 * trs_lgcn_adam: torch.optim.Adam's rule (no amsgrad, no weight decay) on every one of the n elements of a dense table,
 *   one launch:  m += (1-b1)(g-m);  v = v*b2 + ((1-b2) g) g;  p += (-(lr / (1-b1^t)) m) / (sqrt(v) / sqrt(1-b2^t) + eps),
 *   t = step_count >= 1.  1 - beta, lr / (1 - b1^t) and sqrt(1 - b2^t) are formed on the host in double from the
 *   hyper-parameters as written (as trs_rows_apply_sparse_adam forms its constants), then rounded to fp32.
 *   TRS_E_ARG, nothing launched: n < 0; step_count < 1; lr or eps not finite or < 0; a beta outside [0, 1); with n > 0 a
 *   NULL array.  n == 0: TRS_OK, nothing launched. */
#define TRS_LGCN_SEG 512 /* neighbours per segment of trs_lgcn_propagate */
int trs_lgcn_propagate(const float* in_rows_dev, int64_t n_in, int32_t D, const trs_csr* nbr,
                       const float* dinv_out_dev, const float* dinv_in_dev, const float* add_rows_dev, float scale,
                       float* out_rows_dev, int64_t n_out, int32_t accumulate, int32_t* err_flag_dev, void* stream);
int trs_lgcn_adam(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n,
                  float lr, float beta1, float beta2, float eps, int64_t step_count, void* stream);

/* ------------------------------------------------------------------- EASE (fit_ease) */
/* Embarrassingly shallow autoencoder (Steck, WWW 2019): an item-item model with a closed form.  Added without touching
 * an existing signature or struct.
 *
 *   X       the binary n_users x n items matrix of the DISTINCT (user, item) pairs of a CSR (repeated interactions
 *           count once: Steck's definition; a sparse matrix built by summing duplicates would differ on such data)
 *   A       = X^T X + lambda I, lambda > 0: symmetric positive definite, eigenvalues >= lambda
 *   P       = A^-1
 *   B[i][j] = -P[i][j] / P[j][j] for i != j, B[i][i] = 0 (column j divided by its own diagonal entry: not symmetric)
 *   score(u, i) = sum_{j in hist(u)} B[j][i]: the score row of a user is the sum of the B rows of the user's items
 *
 * fp64 matrices are (nbar, nbar) row-major with row stride nbar = n rounded up to a multiple of TRS_EASE_NB.
 *
 * trs_ease_gram: A from the user -> items CSR hist (rows: sorted, distinct item ids).  A[i][j] = the number of users
 *   holding both i and j, formed by fp64 atomic adds of 1.0 (integers below 2^53: exact in any order, so the result
 *   does not depend on the launch), then A[i][i] += lambda with one rounding.  Padding (index >= n): 1 on the diagonal,
 *   0 elsewhere, so the padded matrix is SPD and its inverse is P beside an identity block.  An item id outside [0, n)
 *   is never used as an address: the pair is skipped and bit 0 of *err_flag_dev (may be NULL) is set.
 * trs_ease_invert: P = A^-1 in place, with one workspace of trs_ease_invert_workspace_bytes(n) = nbar * nbar * 8 bytes.
 *   Only the lower triangle of A is read.  Blocked Cholesky route, block size NB = TRS_EASE_NB, every launch on
 *   `stream`, no host synchronisation:
 *     1. right-looking factorisation: per block column k the diagonal block A_kk = L_kk L_kk^T and W_kk = L_kk^-1 (one
 *        workgroup, in LDS), the panel L_ik = A_ik W_kk^T, the trailing update A_ij -= L_ik L_jk^T for i >= j > k;
 *     2. M = L^-1 by block forward substitution: M_kk = W_kk, M_ik = -W_ii sum_{j=k}^{i-1} L_ij M_jk;
 *     3. P = M^T M (lower tiles, then the mirror image: P is exactly symmetric).
 *   Every product runs on one fp64 matrix-core GEMM kernel with a fixed K order: the same input gives the same bits.
 *   A pivot that is not positive and finite sets bit 0 of *err_flag_dev (required) and is replaced by 1.
 *   Knob EASE_STAGES (timing only): bits 0 / 1 / 2 run phase 1 / 2 / 3; three calls with 1, 2 and 4 on the same
 *   matrix and workspace are one inversion.
 * trs_ease_weights: B (n, n) fp32 row-major, row stride n, from P: the division in fp64, rounded to fp32 once; the
 *   diagonal exactly 0.
 * trs_ease_scores: out (n_rows, n) fp32; out[r] = sum of B[j] over the items j of row rows[r] of hist, in fp32, in
 *   ascending CSR position from 0, one add per item (no fused multiply-add, never split across threads): a sequential
 *   float32 loop reproduces it bit for bit.  An empty history gives a row of zeros.  rows may repeat.  A row index
 *   outside the CSR counts as an empty history and an item id outside [0, n) is skipped; both set bit 0 of
 *   *err_flag_dev (may be NULL).
 * TRS_E_ARG, nothing launched: n outside 1..TRS_EASE_NMAX; lambda not finite or <= 0; a NULL matrix, workspace, CSR or
 *   CSR array; hist->n_rows != n_users (trs_ease_gram); a workspace that is too small; a NULL err_flag
 *   (trs_ease_invert).  trs_ease_scores with n_rows == 0: TRS_OK, nothing launched. */
#define TRS_EASE_NB 64      /* block size of trs_ease_invert; fp64 matrices are padded to a multiple of it */
#define TRS_EASE_NMAX 32768 /* largest catalogue: 2 x 8.6 GB fp64 plus 4.3 GB fp32 */
int trs_ease_gram(const trs_csr* hist, int64_t n_users, int64_t n, double lambda, double* A_out_dev,
                  int32_t* err_flag_dev, void* stream);
int64_t trs_ease_invert_workspace_bytes(int64_t n);
int trs_ease_invert(double* A_inout_dev, int64_t n, void* workspace_dev, int64_t workspace_bytes, int32_t* err_flag_dev,
                    void* stream);
int trs_ease_weights(const double* P_dev, int64_t n, float* B_out_dev, void* stream);
int trs_ease_scores(const float* B_dev, int64_t n, const trs_csr* hist, const int64_t* rows_dev, int64_t n_rows,
                    float* out_dev, int32_t* err_flag_dev, void* stream);

/* ------------------------------------------------------------------- item kNN (fit_itemknn) */
/* Sparse item-item neighbourhood model: co-occurrence similarities, K neighbours kept per item.  Nothing of size n^2 is
 * allocated, so it takes catalogues EASE cannot.  Added without touching an existing signature or struct.
 *
 *   X        the binary n_users x n matrix of the DISTINCT (user, item) pairs, as for EASE
 *   U_i      the users of item i, n_i = |U_i|
 *   c(i, j)  = |U_i and U_j|, an exact integer
 *   sim(i, j) from the integers (c, n_i, n_j) and the shrinkage h >= 0, in fp64 with every operation rounded once
 *            (IEEE division and square root, no fast-math intrinsic, no fused multiply-add), then rounded to fp32 once;
 *            a float64 numpy expression reproduces it bit for bit:
 *     TRS_KNN_COSINE       c / (sqrt((double)n_i * (double)n_j) + h)       (the product is exact below 2^53)
 *     TRS_KNN_JACCARD      c / ((double)(n_i + n_j - c) + h)
 *     TRS_KNN_CONDITIONAL  c / ((double)n_i + h)                           (P(j | i): not symmetric)
 *     TRS_KNN_COUNT        c                                               (h is ignored)
 *   neighbours of i: the candidates are the j != i with c(i, j) > 0; row i keeps the K candidates with the largest key,
 *            key = (fp32 similarity descending, j ascending): the key of trs_topk.
 *   THIS PROJECT PRUNES PER ROW: row i votes for its own K nearest items.  (Some libraries keep, per column j, the K
 *   rows with the largest sim(i, j) instead; with a symmetric similarity that is the transposed lists, and the scores
 *   differ.)
 *   score(u, j) = sum of W[i][j] over the items i of hist(u) whose list holds j, accumulated in fp32 from 0, in
 *            ascending CSR position of i, one add per term (no float atomics): a sequential float32 loop reproduces it
 *            bit for bit.  An empty history gives zeros.
 *
 * trs_knn_build: hist = user -> sorted distinct items (n_users rows), inv = item -> sorted distinct users (n rows), the
 *   two CSRs of the same pairs.  Outputs in ELL form, in key order: nbr_ids_out (n, K) int32 with -1 beyond the row's
 *   candidates, nbr_w_out (n, K) fp32 with 0 there.  One launch on `stream` behind a memset of the workspace
 *   (trs_knn_build_workspace_bytes(n, K) bytes: a counter that hands out the items).  The columns are processed in
 *   tiles of TRS_KNN_TILE ids whose 32-bit counters live in LDS; the columns a tile sees are remembered in a list of
 *   TRS_KNN_TOUCHED entries, beyond which the tile is swept.  The counts are integer adds and the selection is by a
 *   total order: the same input gives the same bits, call after call.  An item id outside [0, n) or a user id outside
 *   [0, n_users) is never used as an address: it is skipped and bit 0 of *err_flag_dev (may be NULL) is set.
 * trs_knn_scores: out (n_rows, n) fp32 dense score rows of the rows rows[r] of hist, by the rule above; rows may
 *   repeat.  A row of nbr_ids must list a column at most once (trs_knn_build's output does).  A row index outside the
 *   CSR counts as an empty history; an item id outside [0, n) and a neighbour id other than -1 outside [0, n) are
 *   skipped; all three set bit 0 of *err_flag_dev (may be NULL).
 * TRS_E_ARG, nothing launched: n outside 1..2^31-1 (trs_knn_scores: more than 65 535 column tiles of 8 192); K outside
 *   1..TRS_KNN_KMAX; an unknown kind; a shrinkage that is not finite or < 0; a NULL array, CSR or CSR array;
 *   hist->n_rows != n_users or inv->n_rows != n (trs_knn_build); a NULL or too small workspace.  trs_knn_scores with
 *   n_rows == 0: TRS_OK, nothing launched. */
#define TRS_KNN_COSINE 0
#define TRS_KNN_JACCARD 1
#define TRS_KNN_CONDITIONAL 2
#define TRS_KNN_COUNT 3
#define TRS_KNN_KMAX 128      /* largest K: the bound of trs_topk's kin, the retrieval kernels */
#define TRS_KNN_TILE 16384    /* column ids per tile of trs_knn_build: 64 KiB of 32-bit counters in LDS */
#define TRS_KNN_TOUCHED 512   /* entries of the touched list of a tile; a tile that sees more columns is swept */
int64_t trs_knn_build_workspace_bytes(int64_t n, int32_t K);
int trs_knn_build(const trs_csr* hist, const trs_csr* inv, int64_t n_users, int64_t n, int32_t kind, double shrinkage,
                  int32_t K, int32_t* nbr_ids_out_dev, float* nbr_w_out_dev, void* workspace_dev,
                  int64_t workspace_bytes, int32_t* err_flag_dev, void* stream);
int trs_knn_scores(const int32_t* nbr_ids_dev, const float* nbr_w_dev, int64_t n, int32_t K, const trs_csr* hist,
                   const int64_t* rows_dev, int64_t n_rows, float* out_dev, int32_t* err_flag_dev, void* stream);

/* ------------------------------------------------- exact ranks (rank_items / evaluate_ranks) */
/* Where given items land in a user's full ranking.  Added without touching an existing signature or struct.
 *   v(u, i)    the fp32 value trs_retrieve_topk ranks by: the Linear score / the FM logit z = (acc + ucon_u) + c_i, acc the
 *              fp32 FMA chain over the padded factors in that kernel's order (bit-identical: the target values are
 *              computed by the same MFMA sequence over gathered rows).
 *   key(u, i)  value descending, ties by ascending item id (the key of trs_topk / trs_retrieve_topk).
 *   C_u        all n_items items; with `seen`, without the items of seen row u.
 *   rank(u, t) = #{ i in C_u, i != t : key(u, i) > key(u, t) }, 0-based, int64.  t may itself be a seen item: its rank
 *              is then its position among C_u + {t}.  A user's other targets compete like any other item.  For t in C_u
 *              and k <= TRS_RETRIEVE_KMAX: trs_retrieve_topk(u, k, seen) returns t at position r  <=>  rank(u, t) == r.
 * users (n_q) int64 dense query users; targets: CSR with n_rows == n_q, row q = the targets of query q (dense item ids,
 * sorted, distinct; a user may be queried more than once).  seen (optional): indexed by dense user id, as in
 * trs_retrieve_topk.  Outputs, one entry per target in CSR order (targets->off[n_q] entries): ranks_out int64;
 * values_out (optional) fp32 v(u, t) in the scorer's output units as trs_retrieve_topk writes its scores (Linear: v,
 * FM: sigmoid(v)).  A user outside the table gets rank -1 (value -inf) for all of its targets and is never used as an
 * address; so does a target outside [0, n_items) (callers validate ids before the call).
 * workspace: trs_item_ranks_workspace_bytes(n_q, targets->off[n_q]) bytes = 8 * (n_q + 1) + 8 per target.  The target
 * count lives on the device: the call reads targets->off[n_q] back (8 bytes, one stream synchronisation) after the
 * checks that need no device, then launches two kernels: the target keys, and the counting pass — the tile loop of
 * trs_retrieve_topk over rows of (query, target) with `count += key > target key` as its epilogue, the item splits'
 * partial counts added to ranks_out by 64-bit integer atomics (deterministic).  Knob RANKS_STAGES (timing only): 1 runs
 * the key launch alone, 2 the counting launch alone on the keys a call before left in the same workspace (ranks_out is
 * then added to, not reset), 3 (default) both.
 * TRS_E_ARG, nothing launched: tables NULL or without a user table; net not TRS_NET_LINEAR / TRS_NET_FM; n_q < 0; D
 * outside 1..TRS_RETRIEVE_DMAX; fold_dev NULL or fold_bytes < trs_item_fold_bytes; targets NULL, with a NULL array or
 * with n_rows != n_q; a seen CSR with a NULL array; with n_q > 0 a NULL users / ranks_out or a workspace that is NULL or
 * below trs_item_ranks_workspace_bytes(n_q, 0); after the read-back a workspace below the full size.  n_q == 0 or no
 * target: TRS_OK, nothing launched. */
int64_t trs_item_ranks_workspace_bytes(int64_t n_q, int64_t n_targets);
int trs_item_ranks(int net, const trs_tables* tables, const void* fold_dev, int64_t fold_bytes,
                   const int64_t* users_dev, int64_t n_q, const trs_csr* targets, const trs_csr* seen,
                   int64_t* ranks_out_dev, float* values_out_dev, void* workspace_dev, int64_t workspace_bytes,
                   void* stream);

/* ------------------------------------- diversified re-ranking (recommend_diverse / evaluate_diversity) */
/* Greedy Maximal-Marginal-Relevance (MMR; Carbonell & Goldstein, SIGIR 1998) selection of k entries out of each query's
 * candidate pool, and the intra-list diversity of given lists.  Added without touching an existing signature or struct.
 * Inputs per query: a pool of N entries, 1 <= N <= TRS_RETRIEVE_KMAX, in the order trs_retrieve_topk returned them: ids
 * p_0 .. p_{N-1} (int64; -1 = "no item", which trs_retrieve_topk only writes as a suffix) and their scores v_j (fp32, the
 * scorer's output units); X, a trs_neighbour_fold buffer of the item side (cosine or dot) of (n_items, D); lambda in
 * [0, 1].  Pool positions are "entries" below; every operation is a separately rounded fp32 operation.
 *   valid      entry j is valid iff 0 <= p_j < n_items; n_valid = the number of valid entries.  An id >= n_items (or
 *              below -1) is never used as an address: the entry is invalid and bit 0 of *err_flag_dev (may be NULL) is set.
 *   relevance  v_min / v_max = the smallest / largest v over the valid entries (scan in ascending position with < / >
 *              from the first valid entry); rel_j = (v_j - v_min) / (v_max - v_min), or 0 for all j when v_max == v_min.
 *              Then, along the valid entries in ascending position, rel_j <- rel_j < rel_prev ? rel_j : rel_prev:
 *              relevance is non-increasing along the pool, so a last-bit non-monotonicity of the fp32 sigmoid cannot
 *              reorder what trs_retrieve_topk ordered by the logit.
 *   sim        sim(x, y) = <X_x, X_y> in fp32; the order of the sum (and whether products are fused into it) is free.
 *   a, b       a = 1.0f - lambda, b = lambda.
 *   pick 0     the first valid entry (position 0 of a pool as trs_retrieve_topk writes it), when n_valid > 0.
 *   pick t>=1  for every unselected valid entry j: pen_j = the largest sim(p_j, p_s) over the selected s (running
 *              maximum from -inf with >: a NaN similarity is ignored), m_j = a * rel_j - b * pen_j (two products, one
 *              difference: three roundings).  The pick is the entry with the largest m_j; ties (-0.0 = +0.0) go to the
 *              lowest position, and a NaN ranks below every number: scan in ascending position, j replaces the best so
 *              far iff m_j is a number and (the best so far is a NaN or m_j > it).
 * Outputs for 1 <= k <= N, picks in pick order: ids_out (n_q, k) int64; scores_out (n_q, k) fp32, the picked entries'
 * original v; pos_out (n_q, k) int32 or NULL, their pool positions.  Positions from min(k, n_valid) on hold -1, -inf and
 * -1.  lambda = 0 therefore returns the first k valid pool entries in pool order.
 * One launch, one workgroup per query: the pool's rows are gathered once into registers, each step hands the last pick's
 * row to every entry through LDS — k * N * Dp multiply-adds per query instead of the N^2 * Dp of a similarity matrix.
 * Deterministic (no float atomics).
 * TRS_E_ARG, nothing launched: n_q < 0 (or >= 2^31); N or k outside 1..TRS_RETRIEVE_KMAX; k > N; lambda outside [0, 1] or
 * not a number; D outside 1..TRS_RETRIEVE_DMAX; n_items < 1; fold_bytes != trs_item_fold_bytes(n_items, D); with n_q > 0 a
 * NULL nfold / pool_ids / pool_scores / ids_out / scores_out.  n_q == 0: TRS_OK, nothing launched. */
int trs_mmr_rerank(const void* nfold_dev, int64_t fold_bytes, int64_t n_items, int32_t D, const int64_t* pool_ids_dev,
                   const float* pool_scores_dev, int64_t n_q, int32_t N, int32_t k, float lambda, int64_t* ids_out_dev,
                   float* scores_out_dev, int32_t* pos_out_dev, int32_t* err_flag_dev, void* stream);
/* Intra-list diversity of the lists ids (n_q, k) int64, 1 <= k <= TRS_RETRIEVE_KMAX, over the rows of the same kind of
 * buffer: ild_out[q] (float64) = the mean over the unordered pairs {x, y} of valid entries (0 <= id < n_items; an entry
 * counts once per position, also when an id repeats) of 1 - sim(x, y); sim in fp32 as above, 1 - sim and the sum in
 * float64 in a fixed order; 0.0 with fewer than two valid entries.  An id outside [0, n_items) is never used as an address.
 * TRS_E_ARG, nothing launched: n_q, k, D, n_items, fold_bytes as above; with n_q > 0 a NULL nfold / ids / ild_out.
 * n_q == 0: TRS_OK, nothing launched. */
int trs_list_ild(const void* nfold_dev, int64_t fold_bytes, int64_t n_items, int32_t D, const int64_t* ids_dev,
                 int64_t n_q, int32_t k, double* ild_out_dev, void* stream);

/* ------------------------------------------------------------------------------- in-batch softmax (fit) */
/* Training loss of fit(loss='softmax') for the Linear / FM scorers (Yi et al., RecSys 2019).  Batch
 * rows i < B are (user u_i, positive p_i, metadata m_i) of a trs_batch (neg / neg_meta unused).  With
 *   S_j = item_pj + sum_m meta_m[m_jm]      c_j = item_lin_pj (Linear),
 *                                           c_j = item_lin_pj + sum_m meta_lin_m + 1/2 (|S_j|^2 - |item|^2 - sum_m |meta_m|^2) (FM)
 * the adjusted logits are zh_ij = (<U_ui, S_j> + c_j) / tau - L_j (the user-side 1-wide term cancels in a row softmax),
 * L_j = logq[p_j] when a log-Q table is given (else 0), and zh_ij = -inf for j != i with p_j == p_i (accidental hits).
 *   loss_i = logsumexp_j zh_ij - zh_ii;   G_ij = (P_ij - [i == j]) / B,  P = row softmax of zh.
 * One step, all on `stream`:
 *   trs_softmax_stage                                Q (B, Dq) = user rows with a ones column at Dp, K (B, Dq) = S
 *                                                    rows, cc_j = c_j / tau - L_j, item ids;
 *   for row chunks [r0, r0 + R):  Z = Q[r0:] K^T     trs_gemm_f32(0, 1, R, B, Dp, lda = ldb = Dq);
 *                                 trs_softmax_rows   row losses and G over Z in place;
 *                                 dQ[r0:] = G K      trs_gemm_f32(0, 0, R, Dp, B, ldb = ldc = Dq);
 *                                 dK (+)= G^T Q[r0:] trs_gemm_f32(1, 0, B, Dq, R, beta = 0 on the first chunk, else 1);
 *   trs_softmax_grads                                gradient rows of the batch mean and loss_sum += sum_i loss_i.
 * Dp = D rounded up to a power of two >= 16, Dq = Dp + 4.  Workspace (trs_softmax_workspace_bytes(B, D) bytes, 16-byte
 * aligned), blocks of 4-byte words each starting at a multiple of 64 words: Q, K, dQ, dK (B * Dq each) | cc (B) |
 * row losses (B) | item ids (B, int32).  Every entry point returns TRS_E_ARG (-1) for NULL tables / batch / ids /
 * workspace, B < 1, D < 1, tau <= 0 or not finite, or a workspace smaller than trs_softmax_workspace_bytes(B, D).
 * An id outside its table sets bit 0 of batch->err_flag_dev (its staged row is zero; no gradient row is applied to it). */
int64_t trs_softmax_workspace_bytes(int64_t B, int32_t D);
/* logq_dev: (n_items) fp32 log q of every item, or NULL = no log-Q correction.  Needs n_items < 2^31. */
int trs_softmax_stage(int net, const trs_tables* tables, const trs_batch* batch, float tau, const float* logq_dev,
                      void* workspace_dev, int64_t workspace_bytes, void* stream);
/* Rows [row0, row0 + n_rows) of the logits: z_dev (n_rows, B) fp32 (z_bytes >= n_rows * B * 4) holds Z of those rows
 * and receives G; writes loss_i to the workspace.  No atomics: bit-identical from run to run. */
int trs_softmax_rows(float* z_dev, int64_t z_bytes, int64_t row0, int64_t n_rows, int64_t B, int32_t D, float tau,
                     void* workspace_dev, int64_t workspace_bytes, void* stream);
/* From dQ, dK of the workspace, per batch position j (fields f: 0 = user, 1 = positive item, 2+m = metadata column m):
 *   grad_rows (2+M, B, D): f0 dQ_j / tau;  f1 dK_j / tau (+ FM: dc_j (S_j - item_pj));  f2+m dK_j / tau (+ FM:
 *   dc_j (S_j - meta_m[m_jm])), with dc_j = sum_i G_ij / tau = dK_j[Dp] / tau;
 *   grad_lin (2+M, B): f0 = 0 (the user-side 1-wide term has no gradient, its rows are still touched), f1 = dc_j,
 *   f2+m = dc_j (FM) or 0 (Linear: no 1-wide metadata tables).
 * The uncoalesced COO values of the tables' gradients, as trs_score_fwd_bwd stages them.  grad_rows / grad_lin both
 * NULL: the loss sum only (evaluation).  loss_sum_dev += sum_i loss_i in one fixed order by one thread (no atomics). */
int trs_softmax_grads(int net, const trs_tables* tables, const trs_batch* batch, float tau, const void* workspace_dev,
                      int64_t workspace_bytes, float* grad_rows_dev, float* grad_lin_dev, float* loss_sum_dev,
                      void* stream);

/* ------------------------------------------------------------------------------------- MLP (a4, a7) */
/* Activations of the MLP are kept for both scoring passes stacked: rows [0,B) = positive pass, rows [B,2B) =
 * negative pass ("passes" = 2).  BatchNorm1d statistics are per pass (the reference calls net.forward twice,
 * model.py:171-185).  Workspaces are caller-allocated fp32 arrays of the size the *_workspace_* helpers return. */

/* x0 = [user[u] | item[i] | meta_0[..] | ...] (collaborative/mlp.py:93-105): positive pass into rows [0,B) of x and,
 * when passes == 2, the negative pass into rows [B,2B); row stride ld >= (2+M)*D elements.  x_dev (fp32) and/or
 * x_bf16_dev (bf16, RNE: the operand image of the bf16-resident GEMMs) — either may be NULL. */
int trs_mlp_gather_concat(const trs_tables* tables, const trs_batch* batch, int32_t passes, float* x_dev,
                          void* x_bf16_dev, int64_t ld, void* stream);

/* MLP layer 0 as ONE launch — the "concat-GEMM": y = [user[u] | item[i] | meta_m[..]] W^T + bias with the embedding gather
 * inside the GEMM's A-operand load (replaces the gathers and the two torch.cat of collaborative/mlp.py:93-105 AND
 * fcs[0] of :107; trs_mlp_gather_concat + trs_gemm_* remain for the shapes this entry point does not take).  Rows as in
 * trs_mlp_gather_concat (passes == 2: positive pass then negative pass).  bf16 = 0: W (N, (2+M)D) fp32, y fp32 — the
 * fp32-MFMA LDS-DMA kernel whose A pieces are addressed by id; bf16 = 1: W = the bf16 image of the weight, y fp32
 * (y_dev) or bf16 (y_bf16_dev), fp32 accumulation — table rows rounded to bf16 (RNE) while they are staged.  bn_part as
 * in trs_gemm_f32 (per 128-row chunk).  x_dev / x_bf16_dev (optional, row stride ldx): the x0 image (fp32 for bf16 = 0,
 * bf16 for bf16 = 1) that the weight-gradient GEMM of the backward pass reads, written as a by-product by the workgroups
 * of column block 0 — bit for bit what trs_mlp_gather_concat writes.
 * Returns 0, a negative error, or 1 = shape not taken (int32 ids, B and N multiples of 256, D a multiple of 64 (bf16) /
 * 32 (fp32), at least 256 tiles of 256 x 256, 16-byte aligned operands): nothing was launched. */
int trs_mlp_gather_gemm1_fwd(const trs_tables* tables, const trs_batch* batch, int32_t passes, int32_t bf16,
                             const void* W_dev, int64_t ldw, const float* bias_dev, int64_t N, float* y_dev,
                             void* y_bf16_dev, int64_t ldy, float* bn_part_dev, float* x_dev, void* x_bf16_dev,
                             int64_t ldx, void* stream);

/* SGD on every embedding table of an MLP step, straight from d x0 = the input gradient of the first layer ((2B, ld);
 * rows [0,B) positive pass, [B,2B) negative pass; column block f = field f of x0; fp32 OR bf16 — exactly one of
 * dx0_dev / dx0_bf16_dev): W[row] -= lr * (sum of the d x0 segments of the row's references).  Replaces the sparse COO
 * gradients of the embedding tables + optimizer.step() (model.py:197-198) for the MLP scorer.  Two launches: user / item
 * rows (the user's two passes added in registers; references flagged alone in their batch — user_dup_flags_dev (B),
 * item_dup_flags_dev (B,2) from trs_epoch_flags / trs_epoch_presort, both optional — are plain read-modify-writes, the
 * rest float atomics) and the metadata tables (every workgroup owns a range of categories, sums their references in LDS
 * and applies each row once).  Needs D % 4 == 0, ld % 4 == 0 and metadata tables small enough for the owner-computes
 * form: trs_mlp_embed_sgd_update_supported(tables) != 0. */
int trs_mlp_embed_sgd_update_supported(const trs_tables* tables);
int trs_mlp_embed_sgd_update(const trs_tables* tables, const trs_batch* batch, const float* dx0_dev,
                             const void* dx0_bf16_dev, int64_t ld, float lr, const uint8_t* user_dup_flags_dev,
                             const uint8_t* item_dup_flags_dev, void* stream);

/* C(M,N) = alpha * op(A)(M,K) * op(B)(K,N) + beta * C [+ bias(N) on every row], fp32 in / fp32 accumulate on
 * v_mfma_f32_32x32x2_f32 (an exact fp32 FMA chain).  Row-major; transA: 0 = A stored (M,K), 1 = stored (K,M);
 * transB: 0 = B stored (K,N), 1 = stored (N,K).  Replaces aten::addmm / mm under nn.Linear and its autograd
 * (collaborative/mlp.py:107-113): forward y = x W^T (0,1), dgrad dx = dy W (0,0), wgrad dW = dy^T x (1,0; split-K
 * over workgroups with a fixed-order slab reduce).  workspace: trs_gemm_f32_workspace_bytes(M,N,K) bytes. */
int64_t trs_gemm_f32_workspace_bytes(int64_t M, int64_t N, int64_t K);
int trs_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, float alpha, const float* A_dev,
                 int64_t lda, const float* B_dev, int64_t ldb, float beta, float* C_dev, int64_t ldc,
                 const float* bias_dev, float* bn_part_dev, void* workspace_dev, int64_t workspace_bytes,
                 void* stream);
/* bn_part_dev (optional, forward GEMMs): fused BatchNorm batch statistics of the output — per 128-row tile t and
 * column the mean and the sum of squared deviations from it, written to bn_part[(t*2 + {0,1})*N + col]; combine with
 * trs_bn_stats_finalize(chunk_rows = 128).  Requires beta == 0; disables split-K. */

/* Same interface and storage (fp32 in, fp32 out); the operands are rounded to bf16 (round-to-nearest-even) as they are
 * staged and multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation — the `use_amp=True` mode (the reference's
 * CUDA-only fp16 autocast, model.py:86-88,280, becomes bf16 inputs / fp32 accumulate: no loss scaling needed). */
int trs_gemm_bf16(int transA, int transB, int64_t M, int64_t N, int64_t K, float alpha, const float* A_dev,
                  int64_t lda, const float* B_dev, int64_t ldb, float beta, float* C_dev, int64_t ldc,
                  const float* bias_dev, float* bn_part_dev, void* workspace_dev, int64_t workspace_bytes,
                  void* stream);

/* bf16-RESIDENT GEMM of the use_amp path (activations and weight images already stored as bf16 in HBM; fp32
 * accumulation and fp32 output; same epilogue options as trs_gemm_f32).  tn = 0: C(M,N) = alpha * A(M,K) B(N,K)^T, both
 * operands k-contiguous (forward with W, dgrad with the transposed weight image); tn = 1: C(M,N) = alpha * A(K,M)^T
 * B(K,N) (wgrad dW = dy^T x: both operands "one row per sample"; fragments come out of the transposing LDS read
 * ds_read_b64_tr_b16).  M, N multiples of 128, K a multiple of 64, 16-byte aligned rows (lda, ldb in bf16 elements,
 * multiples of 8).  Output: C_dev (fp32) or, when C_dev is NULL, C_bf16_dev (the value rounded to bf16: the forward
 * outputs y_l and the input gradients dx_l of the bf16-resident path, like autocast's half-precision linear outputs;
 * the fused BatchNorm statistics still come from the fp32 accumulators).  Replaces the reference's autocast `linear` (model.py:86-88,192-195; SURVEY 8a7: bf16 inputs, fp32
 * accumulate, no loss scaling). */
int64_t trs_gemm_bf16in_workspace_bytes(int64_t M, int64_t N, int64_t K);
int trs_gemm_bf16in(int tn, int64_t M, int64_t N, int64_t K, float alpha, const void* A_dev, int64_t lda,
                    const void* B_dev, int64_t ldb, float beta, float* C_dev, void* C_bf16_dev, int64_t ldc,
                    const float* bias_dev, float* bn_part_dev, void* workspace_dev, int64_t workspace_bytes,
                    void* stream);
/* dst (rows, cols) bf16 copy and/or dst_t (cols, rows) transposed bf16 copy of an fp32 matrix (either may be NULL):
 * the per-step refresh of the weight images the bf16-resident GEMMs read. */
int trs_f32_to_bf16(const float* src_dev, int64_t rows, int64_t cols, int64_t ld, void* dst_dev, void* dst_t_dev,
                    void* stream);
/* The same for n (1..8) matrices in ONE launch — every layer's weight images of an MLP step.  The arrays are host arrays
 * of n entries (device pointers / sizes per matrix); dst_dev[k] or dst_t_dev[k] may be NULL. */
int trs_f32_to_bf16_multi(int32_t n, const float* const* src_dev, const int64_t* rows, const int64_t* cols,
                          const int64_t* ld, void* const* dst_dev, void* const* dst_t_dev, void* stream);

/* Train-mode BatchNorm1d statistics of y (passes*rows_per_pass, H) per pass: mean_out/var_out (passes,H), biased
 * variance (chunked two-pass + Chan combination in fp64).  running_mean/var (H) non-NULL: updated once per pass in
 * pass order with `momentum` and the unbiased variance (torch.nn.BatchNorm1d under collaborative/mlp.py:82,110).
 * workspace: trs_bn_workspace_floats(rows_per_pass, H, passes) floats. */
int64_t trs_bn_workspace_floats(int64_t rows_per_pass, int32_t H, int32_t passes);
int trs_bn_batch_stats(const float* y_dev, int64_t rows_per_pass, int32_t H, int64_t ld, int32_t passes,
                       float momentum, float* mean_out_dev, float* var_out_dev, float* running_mean_dev,
                       float* running_var_dev, float* workspace_dev, void* stream);

/* Second half of trs_bn_batch_stats alone: combine chunk partials (pass, chunk, {mean, M2}, H) of `chunk_rows` rows each
 * (as trs_gemm_* writes them with chunk_rows = 128) into mean/var and update the running statistics. */
int trs_bn_stats_finalize(const float* part_dev, int64_t rows_per_pass, int32_t chunk_rows, int32_t H, int32_t passes,
                          float momentum, float* mean_out_dev, float* var_out_dev, float* running_mean_dev,
                          float* running_var_dev, void* stream);

/* out = relu(((y - mean) / sqrt(var + eps)) * gamma + beta)  (use_bn = 0: out = relu(y)); statistics indexed per
 * pass when stat_passes == passes, shared when stat_passes == 1 (eval mode: running statistics).  out_dev (fp32)
 * and/or out_bf16_dev (bf16 image for the bf16-resident GEMMs; needs H % 4 == 0), same row stride ldo in elements.
 * y_bf16 != 0: y_dev is a bf16 image (written by trs_gemm_bf16in), else fp32.
 * running_mean_dev / running_var_dev (both or neither; need use_bn and stat_passes == passes): the momentum update of
 * the running statistics from mean_dev / var_dev, pass by pass — what trs_bn_stats_finalize does when IT is given the
 * running pointers (same arithmetic, bit for bit); pass them to one of the two, not both.  Done by the forward kernel's
 * first row block, which saves the training step one launch per layer.  num_batches_tracked_dev (one int64, may be NULL;
 * with the running pointers): += passes, BatchNorm1d's batch counter, in the same place.
 * dot_w_dev (H) / dot_bias_dev (1, may be NULL) / dot_out_dev (rows_per_pass * passes): the H -> 1 output layer on the
 * last hidden layer's activations, dot_out[r] = sum_c out[r][c] * dot_w[c] + dot_bias (mlp.py:114); formed from the
 * registers of this launch when a row's columns sit in one wave (H a power of two <= 256, aligned rows) — out_dev and
 * out_bf16_dev may then both be NULL: the activations are not stored at all (trs_bn_relu_backward's outer_xw_dev gives the
 * output layer's weight gradient without them) — and by trs_rowdot on out_dev otherwise (same result up to the order of
 * the sum; an error when out_dev is NULL).
 * (collaborative/mlp.py:108-114) */
int trs_bn_relu_forward(const void* y_dev, int32_t y_bf16, int64_t rows_per_pass, int32_t passes, int32_t H, int64_t ld,
                        int32_t use_bn, int32_t stat_passes, const float* mean_dev, const float* var_dev,
                        const float* gamma_dev, const float* beta_dev, float eps, float* out_dev, void* out_bf16_dev,
                        int64_t ldo, float momentum, float* running_mean_dev, float* running_var_dev,
                        int64_t* num_batches_tracked_dev, const float* dot_w_dev, const float* dot_bias_dev,
                        float* dot_out_dev, void* stream);

/* Backward of relu(bn(y)) in train mode from dx = dL/d(out): dy (same shape), dgamma/dbeta (H) summed over both
 * passes.  use_bn = 0: dy = dx * [y > 0].  dy_colsum_dev (H, may be NULL): column sums of dy = the gradient of the
 * preceding Linear's bias, summed per pass first like trs_colsum.  dy_dev (fp32) and/or dy_bf16_dev (bf16 image for
 * the bf16-resident GEMMs; needs H % 4 == 0), row stride ldd elements.  y_bf16 / dx_bf16 != 0: that input is a bf16
 * image (row strides ld / ldd in elements).  workspace:
 * trs_bn_backward_workspace_floats(...) floats.
 * Synchronised BatchNorm under data parallelism (statistics over the GLOBAL batch): phase 1 only reduces —
 * sums_dev (passes,2,H) receives this rank's sum(d) and sum(d*xhat) per pass, dgamma / dbeta are written; the caller
 * all-reduces sums_dev (SUM) and calls phase 2, which applies with those sums and stat_rows = world * rows_per_pass as
 * the divisor.  phase 0 (sums_dev NULL, stat_rows 0) = both at once on the local batch.
 * Outer-product form (the last hidden layer: its dx is the H -> 1 output layer's input gradient g (x) w, mlp.py:115):
 * dx_dev NULL and outer_g_dev (passes*rows_per_pass) / outer_w_dev (H) given — dx[r][c] = g[r] * w[c] is formed in the
 * kernels and never stored (needs H % 4 == 0).  outer_xw_dev (H, may be NULL; outer form with BatchNorm, phase 0):
 * sum_r g[r] * relu(bn(y))[r][:] = the output layer's weight gradient (what trs_colsum(out, row_weight = g) gives on the
 * stored activations), from the activations the reduce kernel recomputes anyway. */
int64_t trs_bn_backward_workspace_floats(int64_t rows_per_pass, int32_t H, int32_t passes);
int trs_bn_relu_backward(const void* y_dev, int32_t y_bf16, const void* dx_dev, int32_t dx_bf16, int64_t rows_per_pass,
                         int32_t passes, int32_t H,
                         int64_t ld, int64_t ldd, int32_t use_bn, const float* mean_dev, const float* var_dev,
                         const float* gamma_dev, const float* beta_dev, float eps, float* dy_dev, void* dy_bf16_dev,
                         float* dgamma_dev, float* dbeta_dev, float* dy_colsum_dev, float* workspace_dev,
                         int32_t phase, float* sums_dev, int64_t stat_rows, const float* outer_g_dev,
                         const float* outer_w_dev, float* outer_xw_dev, void* stream);

/* out[h] = sum_r w[r] * x[r][h] over the passes*rows_per_pass rows (row_weight NULL: plain column sums): bias
 * gradients and the output layer's weight gradient.  Summed per pass first (identical chunking in both passes), so a
 * negative pass that is the exact negation of the positive one cancels to an exact 0 as in the reference's two
 * separate backward passes.  workspace: trs_colsum_workspace_floats(rows_per_pass, passes, H) floats. */
int64_t trs_colsum_workspace_floats(int64_t rows_per_pass, int32_t passes, int32_t H);
int trs_colsum(const float* x_dev, int64_t rows_per_pass, int32_t passes, int32_t H, int64_t ld,
               const float* row_weight_dev, float* out_dev, float* workspace_dev, void* stream);

/* Output layer H -> 1 (collaborative/mlp.py:85,113): out[r] = x[r] . w + bias[0];  and its dgrad dx[r][h] = g[r]*w[h]. */
int trs_rowdot(const float* x_dev, int64_t rows, int32_t H, int64_t ld, const float* w_dev, const float* bias_dev,
               float* out_dev, void* stream);
int trs_outer(const float* g_dev, const float* w_dev, int64_t rows, int32_t H, float* dx_dev, int64_t ld,
              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_H */
